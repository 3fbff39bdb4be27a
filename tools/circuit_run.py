"""The Boolean-circuit notebook's experiments on CircuitIB (InfoDecomp_Boolean_circuits.ipynb cells 6-7 and 10): Fig. 1 (the
paper's 10-input circuit, beta 1e-3 -> 5) and the six SI circuits of Fig. S1 (beta 1e-3 -> 1), 50 000 steps of 512 rows,
evaluations every 250 steps.  Per circuit one JSON file with the selected-subset sequence (cell 7's 0.1-bit rule), the final
per-gate information (bits, smoothed as cell 6 does), the exhaustive Shapley values of I(X_S; Y) next to it
(dib_amd.subset_information: one launch for all subsets), every selected subset's information and rank among the subsets of its
size (cell 7's check), the group-order check of the paper circuit against the notebook's printed sequence, and the smoothed
curves.  --subset_information True also writes subset_information_<circuit>/subset_information.npz and cell 7's figure.
    python tools/circuit_run.py [--out-dir profiles] [--only fig1|si] [--seed 0] [--subset_information True]
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
    a = ap.parse_args(argv)
    from dib_amd import circuit
    os.makedirs(a.out_dir, exist_ok=True)
    jobs = []
    if a.only in (None, "fig1"):
        jobs.append(("fig1", circuit.PAPER_CIRCUIT, 5.0))
    if a.only in (None, "si"):
        jobs += [(f"si_{'abcdef'[k]}", s, 1.0) for k, s in enumerate(circuit.SI_CIRCUITS)]
    for name, spec, beta_end in jobs:
        rec = run_one(name, spec, beta_end, a.seed,
                      subset_information_dir=os.path.join(a.out_dir, f"subset_information_{name}") if a.subset_information else None)
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
