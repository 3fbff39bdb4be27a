"""Science-level check on the PAPER's 10-input Boolean circuit (reference data.py:21-81 = `train.py --dataset boolean_circuit`;
Murphy & Bassett PNAS 2024 Fig. 1): as beta is annealed the Distributed IB stops paying for the input gates one group at a
time.  The reference notebook complex_systems/InfoDecomp_Boolean_circuits.ipynb holds the outcome of ITS OWN TensorFlow run
as a printed cell output (cell 7: "Sequence of selected subsets: [0 1 2 5 6 7 8 9], [0 1 2 5 7 8 9], [2 5 7 8 9], [2 5 9],
[2 9], [2], []", information threshold 0.1 bits) - i.e. gates {3, 4} are dropped first, then 6, then {0, 1}, then {7, 8},
then 5, then 9 and gate 2 last.  This runs the same circuit through DistributedIBNet.fit (MLP encoders, the train.py
architecture) on a compressed schedule and reports when each gate's KL falls below the threshold for good."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dib_amd

NOTEBOOK_DROP_GROUPS = [(3, 4), (6,), (0, 1), (7, 8), (5,), (9,), (2,)]     # printed by the reference's own TF run


def run(epochs_pre=100, epochs_anneal=1500, seed=0, learning_rate=1e-3, batch_size=128, beta_start=1e-3, beta_end=5.0,
        threshold_bits=0.1):
    """-> (drop_epoch [10] = first epoch after which the gate's KL (bits, 9-epoch running mean) stays below the threshold,
    kl_bits [epochs, 10], loss_bits [epochs], accuracy [epochs], beta [epochs])"""
    d = dib_amd.data.fetch_boolean_circuit()
    x, y = d["x_train"].astype(np.float32), d["y_train"].astype(np.float32)
    m = dib_amd.DistributedIBNet(d["feature_dimensionalities"], [128, 128], [256, 256], 1, feature_embedding_dimension=32,
                                 noise_seed=seed, init_seed=seed, shuffle_seed=seed)
    opt = dib_amd.optimizers.get("adam")
    opt.learning_rate = learning_rate
    m.compile(optimizer=opt, loss=d["loss"], metrics=["accuracy"])
    cb = dib_amd.InfoBottleneckAnnealingCallback(beta_start, beta_end, epochs_pre, epochs_anneal)
    h = m.fit(x, y, epochs=epochs_pre + epochs_anneal, batch_size=batch_size, callbacks=[cb], verbose=False).history
    kl = np.stack([h[f"KL{f}"] for f in range(10)], -1) / np.log(2)
    beta = np.array(h["beta"])
    loss_bits = (np.array(h["loss"]) - beta * kl.sum(-1) * np.log(2)) / np.log(2)
    k = np.ones(9) / 9
    sm = np.stack([np.convolve(kl[:, f], k, mode="same") for f in range(10)], -1)
    above = sm > threshold_bits
    drop = np.array([(np.where(above[:, f])[0].max() + 1) if above[:, f].any() else 0 for f in range(10)])
    return drop, kl, loss_bits, np.array(h["accuracy"]), beta


def group_order_violations(drop, slack=0):
    """pairs (gate a of an earlier notebook group, gate b of a later one) with drop[a] > drop[b] + slack"""
    bad = []
    for i, ga in enumerate(NOTEBOOK_DROP_GROUPS):
        for gb in NOTEBOOK_DROP_GROUPS[i + 1:]:
            bad += [(a, b) for a in ga for b in gb if drop[a] > drop[b] + slack]
    return bad


def subset_information_bits(x, y, backend="host"):
    """I(X_S;Y) in bits of all 2^10 subsets of the uniform truth table, indexed by the bitmask of kept gates (bit i = gate i):
    dib_amd.subset_information (the quantity of Boolean_circuits.ipynb:425-434; the tests use the notebook's own numbers,
    tests/golden/subset_mi.npz).  backend "host" (float64 NumPy, what the CPU tests call) or "device" (one launch)."""
    return dib_amd.subset_information.subset_information(x, y, backend=backend).bits


def info_ceiling_excess(kl_bits, loss_bits, subset_info, entropy_y_bits, kept_threshold_bits=0.02):
    """Data-processing ceiling on every recorded epoch.  With S = the gates whose encoders still transmit
    (KL_i > kept_threshold_bits; KL_i upper-bounds I(U_i;X_i)):
        H(Y) - task loss  <=  I(U;Y)  <=  I(X_S;Y) + sum_{i not in S} KL_i
    (cross-entropy >= H(Y|U); chain rule + I(U_i;Y|.) <= I(U_i;X_i) <= KL_i for the gates outside S).  Returns per epoch
    (H(Y) - loss) - ceiling: positive values are violations (up to the sampling noise of one epoch of reparameterised draws)."""
    kl_bits, loss_bits = np.asarray(kl_bits, dtype=np.float64), np.asarray(loss_bits, dtype=np.float64)
    kept = kl_bits > kept_threshold_bits
    masks = (kept.astype(np.int64) << np.arange(kl_bits.shape[1])).sum(1)
    ceiling = np.array([subset_info[int(m)] for m in masks]) + np.where(kept, 0.0, kl_bits).sum(1)
    return (entropy_y_bits - loss_bits) - ceiling, masks


if __name__ == "__main__":
    import time
    _d = dib_amd.data.fetch_boolean_circuit()
    _info = subset_information_bits(_d["x_train"], _d["y_train"], backend="device")
    # (beta_start = 1e-3, the notebook's value for ITS encoders - two trainable scalars per gate that start informative, mu = +-1 and
    # logvar = -3 - is too strong a bottleneck for MLP encoders that start uninformative: the XOR pair {7, 8} is priced out
    # before the integration network has learnt to use it (accuracy stays at 0.89, profiles/r04p_paper_circuit.txt); with
    # beta_start <= 1e-5, or train.py's own defaults 1e-4 / lr 3e-4 and a longer warm-up, pre-training reaches accuracy 1)
    for kw in (dict(epochs_pre=1000, beta_start=1e-5, seed=2), dict(epochs_pre=500, beta_start=1e-6, seed=4),
               dict(epochs_pre=1000, beta_start=1e-5, seed=0), dict(epochs_pre=1000, beta_start=1e-5, seed=1),
               dict(epochs_pre=1000, beta_start=1e-5, seed=3),
               dict(epochs_pre=2000, beta_start=1e-4, learning_rate=3e-4, epochs_anneal=3000)):   # train.py's defaults, compressed
        t0 = time.time()
        drop, kl, loss, acc, beta = run(**kw)
        print(kw, f"{time.time() - t0:.1f}s", "drop epochs", drop.tolist(), "order", np.argsort(drop, kind="stable").tolist(),
              "violations", group_order_violations(drop), f"acc@pre {acc[kw.get('epochs_pre', 100) - 1]:.3f} loss@pre {loss[kw.get('epochs_pre', 100) - 1]:.3f} "
              f"final KL {kl[-1].sum():.3f} final loss {loss[-1]:.3f} bits", flush=True)
        exc, masks = info_ceiling_excess(kl, loss, _info, _info[1023])
        print(f"   subset-information ceiling: max (H(Y) - loss) - [I(X_S;Y) + sum KL outside S] = {exc.max():+.4f} bits at epoch "
              f"{int(exc.argmax())}; {len(set(masks.tolist()))} distinct kept subsets visited", flush=True)
