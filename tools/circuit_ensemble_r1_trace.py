"""Where the R = 1 CircuitEnsemble step differs from the CircuitIB step: 300 steps of each at the notebook's size
(B = 512, (256, 256, 256)) for a kernel trace, then the host's time to issue a step with the queue never drained.

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o r1 -- python tools/circuit_ensemble_r1_trace.py
The per-kernel table (DIR/**/r1_kernel_stats.csv) is kept as profiles/circuit_ensemble_r1_kernel_stats.csv."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from dib_amd import circuit
    t = circuit.truth_table(circuit.SI_CIRCUITS[2])
    ens = circuit.CircuitEnsemble([t])
    m = circuit.CircuitIB(4)
    tab = m._table(t)
    for _ in range(300):
        ens._step(512, [0.1])
    torch.cuda.synchronize()
    for _ in range(300):
        m._step(tab, 512, 0.1)
    torch.cuda.synchronize()
    for name, fn in (("ensemble", lambda: ens._step(512, [0.1])), ("single", lambda: m._step(tab, 512, 0.1))):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        print(name, "host issue time per step (20 steps, no synchronisation inside): %.1f us" % ((t1 - t0) / 20 * 1e6))


if __name__ == "__main__":
    main()
