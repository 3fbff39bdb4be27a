"""Fixture for the set-transformer notebook's information tracking from the reference NOTEBOOK's own statements, executed on the
NumPy stand-in for TensorFlow (tests/golden/tf_numpy_shim.py), as make_golden_probe_grid.py does.  Run here only:
    python tests/golden/make_golden_st_information.py
  - cell 5's `compute_infos_mus_logvars` (from its `@tf.function` line to `def bhattacharyya_dist_mat`) on small random Gaussian
    batches with known noise;
  - cell 8's information-plane tail (from `bce_series_val = np.float32(bce_series_val) / np.log(2)` to the `info_out` line, the
    `np.savez` block left out) on a synthetic history, scipy.ndimage as `nim`.
The .ipynb is read at generation time only (nothing is copied into this repository).  Writes tests/golden/st_information.npz."""
import json
import os
import sys
import textwrap

import numpy as np
import scipy.ndimage as nim

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tf_numpy_shim as tf  # noqa: E402

NB = "/root/reference/complex_systems/InfoDecomp_Amorphous_plasticity_per_particle_measurements_and_set_transformer.ipynb"


def main():
    nb = json.load(open(NB))
    cells = ["".join(c["source"]) for c in nb["cells"] if c["cell_type"] == "code"]
    c5 = next(c for c in cells if "def compute_infos_mus_logvars" in c)
    src = c5[c5.index("@tf.function\ndef compute_infos_mus_logvars"):c5.index("def bhattacharyya_dist_mat")]
    g = {"tf": tf, "np": np}
    exec(compile(src, "nb:cell5[compute_infos_mus_logvars]", "exec"), g)
    rng = np.random.default_rng(11)
    out = {}
    for k, (n, E, spread) in enumerate([(40, 6, 1.0), (25, 4, 0.3), (2, 3, 1.0)]):
        mus = rng.standard_normal((n, E)) * spread
        logvars = rng.standard_normal((n, E)) * 0.5 - 3.0      # already includes the -3 offset (the notebook adds it first)
        if k == 0:
            mus[1] = mus[0]                                   # a repeated row (neighbourhoods drawn with replacement)
            logvars[1] = logvars[0]
        eps = rng.standard_normal((n, E))
        tf.push_eps([eps])
        lower, upper = g["compute_infos_mus_logvars"](mus, logvars)
        out.update({f"mus{k}": mus, f"logvars{k}": logvars, f"eps{k}": eps, f"lower{k}": np.float64(lower), f"upper{k}": np.float64(upper)})
    big = next(c for c in cells if "set_transformer = tf.keras.Model(inp, x)" in c)
    start = big.index("  bce_series_val = np.float32(bce_series_val) / np.log(2)")
    end = big.index("  plt.figure(figsize=(10, 6))", start)
    body = textwrap.dedent(big[start:end])
    body = body.replace("if save_outputs:", "if False:")
    hist = dict(bce_series_val=list(0.7 - 0.4 * np.linspace(0, 1, 30) + 0.02 * rng.standard_normal(30)),
                acc_series_val=list(0.5 + 0.4 * np.linspace(0, 1, 30) + 0.01 * rng.standard_normal(30)),
                info_bounds=[[a, a + 1.5] for a in 20.0 * np.linspace(1, 0.2, 21) + rng.standard_normal(21)])
    g = {"np": np, "nim": nim, "bce_series_val": list(hist["bce_series_val"]), "acc_series_val": list(hist["acc_series_val"]),
         "info_bounds": list(hist["info_bounds"])}
    exec(compile(body, "nb:cell8[information plane]", "exec"), g)
    out.update(hist_bce=np.asarray(hist["bce_series_val"]), hist_acc=np.asarray(hist["acc_series_val"]),
               hist_info_bounds=np.asarray(hist["info_bounds"]), info_in=np.asarray(g["info_in_full"]),
               info_out=np.asarray(g["info_out"]), acc_plot=np.asarray(g["acc_series_val"][g["plotting_start_ind"]:]))
    np.savez_compressed(os.path.join(HERE, "st_information.npz"), **out)
    print({k: out[k] for k in ("lower0", "upper0", "lower1", "upper1")}, out["info_in"][:3], out["info_out"][:3])


if __name__ == "__main__":
    main()
