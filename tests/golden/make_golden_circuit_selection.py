"""Golden fixture of the Boolean-circuit notebook's read-out: the post-processing statements of the reference notebook
complex_systems/InfoDecomp_Boolean_circuits.ipynb are EXECUTED, not restated -
  * cell 6 from `mutual_information_bounds = np.reshape` up to its first plot (bits, the channel mean of the bounds, the three
    Gaussian smoothings) and
  * cell 7 from `information_threshold = 0.1` up to its print (the cumulative 0.1-bit rule, the "Sequence of selected subsets")
are cut out of the notebook's code cells by their source text at generation time and run on a fixed synthetic history: ten
channels whose bounds fall off one after another in the notebook's group order, with noise, and a noisy BCE series.  Only
the numbers are stored (tests/golden/circuit_selection.npz).  Run in the build container only (/root/reference is absent on
the GPU box):

    python tests/golden/make_golden_circuit_selection.py
"""
import json
import os

import numpy as np
import scipy.ndimage

NB = "/root/reference/complex_systems/InfoDecomp_Boolean_circuits.ipynb"
OUT = os.path.dirname(os.path.abspath(__file__))


def synthetic_history(seed=0, G=10, n_steps=4000, freq=20):
    rng = np.random.default_rng(seed)
    t = np.arange(0, n_steps, freq) / n_steps
    drop = np.array([0.35, 0.36, 0.8, 0.15, 0.16, 0.6, 0.25, 0.45, 0.46, 0.7])   # the notebook's order: {3,4} 6 {0,1} {7,8} 5 9 2
    level = np.array([0.6, 0.6, 1.0, 0.3, 0.3, 0.7, 0.4, 0.5, 0.5, 0.8])
    mid = level[None, :] / (1.0 + np.exp((t[:, None] - drop[None, :]) / 0.02)) + 0.01 * rng.standard_normal((len(t), G))
    mid = np.clip(mid, 0.0, 1.0) * np.log(2)                                               # nats, like estimate_mi_sandwich_bounds
    half = 0.002 * np.abs(rng.standard_normal((len(t), G)))
    bounds = np.stack([mid - half, mid + half], -1).reshape(-1, 2)                         # the notebook's flat list of [lower, upper]
    bce = (0.1 + 0.4 * np.arange(n_steps) / n_steps + 0.05 * rng.standard_normal(n_steps)).astype(np.float32)
    return bounds, bce, G, n_steps, freq


def main():
    cells = ["".join(c["source"]) for c in json.load(open(NB))["cells"] if c["cell_type"] == "code"]
    train = next(s for s in cells if "evaluate_mutual_info_freq = number_training_steps//200" in s and "circuit_specs" not in s)
    a = train.index("mutual_information_bounds = np.reshape")
    post = train[a:train.index("plt.figure", a)]
    select = next(s for s in cells if "information_threshold = 0.1" in s and "print('Sequence of selected subsets:'" in s)
    a = select.index("information_threshold = 0.1")
    select = select[a:select.index("print('Sequence of selected subsets:'", a)]
    bounds, bce, G, n_steps, freq = synthetic_history()
    entropy_y = 0.7578784625383954
    g = {"np": np, "nim": scipy.ndimage, "number_input_gates": G, "number_training_steps": n_steps,
         "evaluate_mutual_info_freq": freq, "mutual_information_bounds": [list(r) for r in bounds],
         "bce_loss_series": list(bce), "entropy_y": entropy_y}
    exec(compile(post, NB, "exec"), g)
    exec(compile(select, NB, "exec"), g)
    subsets = g["input_subsets_above_threshold"]
    assert isinstance(subsets[-1], range)
    masks = np.zeros((len(subsets) - 1, G), dtype=np.int8)
    for k, s in enumerate(subsets[:-1]):
        masks[k, np.asarray(s, dtype=np.int64)] = 1
    np.savez(os.path.join(OUT, "circuit_selection.npz"), bounds_nats=bounds, bce_loss_series=bce, number_training_steps=n_steps,
             evaluate_mutual_info_freq=freq, entropy_y_bits=np.float64(entropy_y), info_in_parts=g["info_in_parts"],
             info_in_full=g["info_in_full"], predictive_information_out=g["predictive_information_out"],
             selected_subset_masks=masks)
    print("Sequence of selected subsets:", subsets)


if __name__ == "__main__":
    main()
