"""Here is my table - where is the information in it?

Writes a small synthetic mixed table (three continuous columns, a count, a 3-level category; the label depends on one continuous
column and on the category) to a temporary .npz and runs it through `python -m dib_amd.train --dataset table`: the reference's
preprocessing (one-hot, quantile transform to a normal on the device), a short beta ramp, and the information every feature's
channel keeps at the end of it.  Needs no download:

    python examples/tabular_dib.py            (needs an MI355X; there is no CPU path)
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dib_amd import train  # noqa: E402


def write_table(path, n=2048, seed=0):
    rng = np.random.default_rng(seed)
    x = np.stack([rng.standard_normal(n), rng.exponential(size=n), 3.0 * rng.standard_normal(n) + 1.0,
                  rng.poisson(2.0, n).astype(float), rng.integers(0, 3, n).astype(float)], 1).astype(np.float32)
    y = (x[:, 0] + 1.5 * (x[:, 4] == 1) - 0.5 > 0).astype(np.int64)
    np.savez(path, x=x, y=y, columns=np.array(["signal", "waiting_time", "noise", "count", "kind"]))


def main(epochs=(4, 12)):
    with tempfile.TemporaryDirectory(prefix="tabular_dib") as tmp:
        path = os.path.join(tmp, "table.npz")
        write_table(path)
        history = train.main(["--dataset", "table", "--table_path", path, "--table_categorical", "kind",
                              "--number_pretraining_epochs", str(epochs[0]), "--number_annealing_epochs", str(epochs[1]),
                              "--beta_start", "1e-3", "--beta_end", "1.0", "--batch_size", "128", "--learning_rate", "1e-3",
                              "--feature_encoder_architecture", "32", "32", "--integration_network_architecture", "64", "64",
                              "--feature_embedding_dimension", "8", "--artifact_outdir", os.path.join(tmp, "artifacts")])
    h = history.history
    print("feature        KL (bits) at the first / last epoch (validation)")
    for f, label in enumerate(["signal", "waiting_time", "noise", "count", "kind"]):
        print(f"{label:14s} {h[f'val_KL{f}'][0] / np.log(2):8.3f}  {h[f'val_KL{f}'][-1] / np.log(2):8.3f}")
    print(f"validation accuracy {h['val_accuracy'][-1]:.3f}")
    return history


if __name__ == "__main__":
    main()
