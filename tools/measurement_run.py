"""Chaos notebook cell 10 end to end on the device: train a measurement partition (dib_amd.MeasurementIB.fit with the
notebook's hyperparameters and its I(U~;X) >= 1 bit stopping rule), symbolise an evaluation trajectory with 100 fixed noise
draws, and characterise the symbols (H(U), CTW entropy rates of 15 window lengths x 5 draws, Schurmann-Grassberger fit) against
the Kolmogorov-Sinai entropy of the system.  Prints one JSON line (and writes it to --out).

    python tools/measurement_run.py --system ikeda [--number-states 12] [--steps 20000] [--out profiles/....json]

--repeats N (the notebook's "20 repeats per number_states"): the N repeats train in lockstep as ONE dib_amd.MeasurementEnsemble
(repeat r: weights seeded --seed + 4 r, noise --seed + r, batches --seed + r; each retires at its own 1 bit), then each is
symbolised and characterised on its own: one JSON line per repeat.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ENTROPY_RATE = {"logistic": 0.5203, "henon": 0.6048, "ikeda": 0.726}   # cell 10's entropy_rate_dict (bits)


def _record(a, h, sym, t_data, t_fit, t_sym, characterize_partition, train_points, repeat=None):
    """the result line of one trained model: its fit history h, its symbols of the evaluation trajectory, their characterisation"""
    info = [float(np.mean(i)) for i in h["info_in"]]
    stopped = bool(info) and info[-1] >= 1.0
    t0 = time.time()
    ch = characterize_partition(sym, 2, number_rand_draws=5, seed=a.seed, ctw_backend=a.ctw_backend)
    t_char = time.time() - t0
    rec = {"system": a.system, "number_states": a.number_states, "alphabet_size": 2, "max_steps": a.steps, "ctw_backend": a.ctw_backend,
           "steps_run": h["steps"], "reached_1_bit": stopped,
           "stopping_step": h["steps"] if stopped else None,
           "info_in_bits_last": info[-1] if info else None, "info_out_bits_last": float(h["info_out"][-1]) if h["info_out"] else None,
           "final_loss": h["loss"][-1], "final_beta": h["beta"][-1],
           "H_U_bits": ch["entropy_single_timestep"], "entropy_rate_bits": ch["entropy_rate"],
           "entropy_rate_err_bits": ch["entropy_rate_err"], "h_KS_bits": ENTROPY_RATE[a.system],
           "symbol_fraction_1": float(sym.mean()), "eval_points": int(len(sym)), "train_points": int(train_points),
           "seconds": {"data": round(t_data, 1), "fit": round(t_fit, 1), "symbolize": round(t_sym, 2), "characterize": round(t_char, 1)},
           "info_in_series_bits": [round(v, 4) for v in info]}
    if repeat is not None:   # (the fit seconds are the whole ensemble's: the repeats train in lockstep)
        rec = {"repeat": repeat, "repeats": a.repeats, **rec}
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--system", default="ikeda", choices=sorted(ENTROPY_RATE))
    ap.add_argument("--number-states", type=int, default=12)
    ap.add_argument("--steps", type=int, default=20_000)
    ap.add_argument("--train-points", type=int, default=1_000_000)
    ap.add_argument("--eval-points", type=int, default=4_000_000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=1, help="train this many repeats as one MeasurementEnsemble; one result per repeat")
    ap.add_argument("--ctw_backend", default="host", choices=("host", "device"),
                    help="where the CTW entropy rates are estimated (dib_amd.ctw.estimate_entropy_windows)")
    a = ap.parse_args(argv)
    import dib_amd
    from dib_amd import chaos_data
    from dib_amd.measurement import MeasurementIB, characterize_partition

    t0 = time.time()
    train = chaos_data.generate_data(a.system, a.train_points, seed=a.seed).astype(np.float32)
    ev = chaos_data.generate_data(a.system, a.eval_points, seed=a.seed + 1).astype(np.float32)
    t_data = time.time() - t0
    if a.repeats > 1:
        from dib_amd import MeasurementEnsemble
        ens = MeasurementEnsemble(a.repeats, input_dimensionality=train.shape[1], number_states=a.number_states, noise_seed=a.seed,
                                  init_seed=a.seed)
        t0 = time.time()
        hs = ens.fit(train, number_training_steps=a.steps, batch_size=2048, learning_rate=3e-4, beta_start=10, beta_end=1e-4,
                     info_eval_data=ev[:1_000_000], evaluate_info_every=a.steps // 100, info_stopping_point=1.0,
                     seeds=[a.seed + r for r in range(a.repeats)])
        t_fit = time.time() - t0
        recs = []
        for r, h in enumerate(hs):
            t0 = time.time()
            sym = ens.symbolize(r, ev, number_averaging_logits=100, seed=a.seed)
            t_sym = time.time() - t0
            recs.append(_record(a, h, sym, t_data, t_fit, t_sym, characterize_partition, len(train), repeat=r))
        lines = [json.dumps(rec) for rec in recs]
        print("\n".join(lines))
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return recs
    m = MeasurementIB(train.shape[1], number_states=a.number_states, noise_seed=a.seed, init_seed=a.seed)
    t0 = time.time()
    h = m.fit(train, number_training_steps=a.steps, batch_size=2048, learning_rate=3e-4, beta_start=10, beta_end=1e-4,
              info_eval_data=ev[:1_000_000], evaluate_info_every=a.steps // 100, info_stopping_point=1.0, seed=a.seed)
    t_fit = time.time() - t0
    t0 = time.time()
    sym = m.symbolize(ev, number_averaging_logits=100, seed=a.seed)
    t_sym = time.time() - t0
    rec = _record(a, h, sym, t_data, t_fit, t_sym, characterize_partition, len(train))
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return rec


if __name__ == "__main__":
    main()
