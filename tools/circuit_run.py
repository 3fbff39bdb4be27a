"""The Boolean-circuit notebook's experiments on CircuitIB (InfoDecomp_Boolean_circuits.ipynb cells 6-7 and 10): Fig. 1 (the
paper's 10-input circuit, beta 1e-3 -> 5) and the six SI circuits of Fig. S1 (beta 1e-3 -> 1), 50 000 steps of 512 rows,
evaluations every 250 steps.  Per circuit one JSON file with the selected-subset sequence (cell 7's 0.1-bit rule), the final
per-gate information (bits, smoothed as cell 6 does), the exhaustive Shapley values of I(X_S; Y) next to it
(dib_amd.subset_information: one launch for all subsets), every selected subset's information and rank among the subsets of its
size (cell 7's check), the group-order check of the paper circuit against the notebook's printed sequence, and the smoothed
curves.  --subset_information True also writes subset_information_<circuit>/subset_information.npz and cell 7's figure.
--ensemble trains the six SI circuits in lockstep on one CircuitEnsemble (every launch of a step shared) and writes the same
records; replica k has the seeds and draws of the sequential run of circuit k, "fit_wall_s" is the shared wall time.
    python tools/circuit_run.py [--out-dir profiles] [--only fig1|si] [--seed 0] [--subset_information True] [--ensemble]
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOTEBOOK_FIG1_SEQUENCE = [[0, 1, 2, 5, 6, 7, 8, 9], [0, 1, 2, 5, 7, 8, 9], [2, 5, 7, 8, 9], [2, 5, 9], [2, 9], [2], []]


def run_one(name, spec, beta_end, seed, steps=50_000, batch_size=512, subset_information_dir=None):
    from dib_amd import circuit, subset_information
    table = circuit.truth_table(spec)
    G = table.shape[1] - 1
    m = circuit.CircuitIB(G, noise_seed=seed, init_seed=seed)
    t0 = time.perf_counter()
    h = m.fit(table, number_training_steps=steps, batch_size=batch_size, beta_start=1e-3, beta_end=beta_end, seed=seed)
    wall = time.perf_counter() - t0
    return record(name, spec, beta_end, seed, h, wall, steps, batch_size, subset_information_dir)


def run_ensemble(jobs, seed, steps=50_000, batch_size=512, subset_information_dir=None):
    """the jobs' circuits as the replicas of one CircuitEnsemble: [(name, record)] in the jobs' order"""
    from dib_amd import circuit
    R = len(jobs)
    ens = circuit.CircuitEnsemble([circuit.truth_table(spec) for _, spec, _ in jobs], init_seeds=[seed] * R, noise_seeds=[seed] * R)
    t0 = time.perf_counter()
    hs = ens.fit(number_training_steps=steps, batch_size=batch_size, beta_start=1e-3, beta_end=[b for _, _, b in jobs],
                 seeds=[seed] * R)
    wall = time.perf_counter() - t0
    return [(name, record(name, spec, beta_end, seed, h, wall, steps, batch_size,
                          subset_information_dir(name) if subset_information_dir else None))
            for (name, spec, beta_end), h in zip(jobs, hs)]


def record(name, spec, beta_end, seed, h, wall, steps, batch_size, subset_information_dir=None):
    """the JSON record of one circuit's fit history h"""
    from dib_amd import circuit, subset_information
    table = circuit.truth_table(spec)
    G = table.shape[1] - 1
    hy = circuit.entropy_bits(table[:, -1])
    ip = circuit.information_plane(h, hy)
    seq = [list(map(int, s)) for s in circuit.selected_subsets(ip["info_in_parts"])[:-1]]
    drop = np.cumprod(ip["info_in_parts"] > 0.1, axis=0).sum(0)
    info = subset_information.subset_information(table[:, :G], table[:, -1])
    shap = info.shapley_values()
    comparison = circuit.subset_comparison(ip["info_in_parts"], table)
    if subset_information_dir is not None:
        subset_information.save_subset_information(info, subset_information_dir, selected=[r["gates"] for r in comparison],
                                                   info_in_full=ip["info_in_full"],
                                                   predictive_information_out=ip["predictive_information_out"])
    rec = {"circuit": name, "circuit_specification": spec, "number_input_gates": G, "beta_start": 1e-3, "beta_end": beta_end,
           "number_training_steps": steps, "batch_size": batch_size, "seed": seed, "entropy_y_bits": hy, "fit_wall_s": round(wall, 3),
           "selected_subsets": seq, "evaluations_in_selected_set_per_gate": drop.tolist(),
           "final_info_per_gate_bits": ip["info_in_parts"][-1].tolist(),
           "max_info_per_gate_bits": ip["info_in_parts"].max(0).tolist(),
           "shapley_values_bits": shap.tolist(), "selected_subset_comparison": comparison,
           "curves": {"evaluation_steps": h["evaluation_steps"].tolist(), "info_in_parts": np.round(ip["info_in_parts"], 5).tolist(),
                      "info_in_full": np.round(ip["info_in_full"], 5).tolist(),
                      "predictive_information_out": np.round(ip["predictive_information_out"], 5).tolist()}}
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--only", choices=["fig1", "si"], default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--subset_information", type=lambda v: str(v).lower() in ("1", "true", "yes", "y", "t"), default=False,
                    help="write subset_information.npz (masks, bits, entropy_y_bits, Shapley values) and cell 7's figure per circuit")
    ap.add_argument("--ensemble", action="store_true", help="the SI circuits as one CircuitEnsemble trained in lockstep")
    ap.add_argument("--steps", type=int, default=50_000)
    a = ap.parse_args(argv)
    from dib_amd import circuit
    os.makedirs(a.out_dir, exist_ok=True)
    jobs = []
    if a.only in (None, "fig1"):
        jobs.append(("fig1", circuit.PAPER_CIRCUIT, 5.0))
    if a.only in (None, "si"):
        jobs += [(f"si_{'abcdef'[k]}", s, 1.0) for k, s in enumerate(circuit.SI_CIRCUITS)]
    sub_dir = (lambda name: os.path.join(a.out_dir, f"subset_information_{name}")) if a.subset_information else None
    lockstep = {}
    if a.ensemble:
        lockstep = dict(run_ensemble([j for j in jobs if j[0] != "fig1"], a.seed, steps=a.steps, subset_information_dir=sub_dir))
    for name, spec, beta_end in jobs:
        rec = lockstep.get(name) or run_one(name, spec, beta_end, a.seed, steps=a.steps,
                                            subset_information_dir=sub_dir(name) if sub_dir else None)
        if name == "fig1":
            sp = importlib.util.spec_from_file_location("paper_circuit_run", os.path.join(ROOT, "tools", "paper_circuit_run.py"))
            pcr = importlib.util.module_from_spec(sp)
            sp.loader.exec_module(pcr)
            rec["notebook_sequence"] = NOTEBOOK_FIG1_SEQUENCE
            rec["sequence_equals_notebook"] = rec["selected_subsets"] == NOTEBOOK_FIG1_SEQUENCE
            rec["group_order_violations_slack1"] = [list(map(int, p)) for p in
                                                    pcr.group_order_violations(rec["evaluations_in_selected_set_per_gate"], slack=1)]
        path = os.path.join(a.out_dir, f"circuit_run_{name}.json")
        with open(path, "w") as f:
            json.dump(rec, f)
            f.write("\n")
        print(name, "wall", rec["fit_wall_s"], "s; selected subsets:", rec["selected_subsets"])
        print("   final info (bits):", np.round(rec["final_info_per_gate_bits"], 3).tolist(), " Shapley (bits):",
              np.round(rec["shapley_values_bits"], 3).tolist())


if __name__ == "__main__":
    main()
