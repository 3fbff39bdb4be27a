"""float64 reference of the compression-scheme matrices (include/dib_compression.h), built on oracle/dib_oracle.py's
encode_feature, bhattacharyya_dist_mat and compression_matrix, imported unchanged."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import dib_oracle as orc  # noqa: E402


def distances(enc):
    """Bhattacharyya distances [n, n] between the Gaussians enc [n, 2E] (mu | logvar), float64"""
    enc = np.asarray(enc, dtype=np.float64)
    E = enc.shape[1] // 2
    return orc.bhattacharyya_dist_mat(enc[:, :E], enc[:, E:], enc[:, :E], enc[:, E:])


def magnitude(enc):
    """A [n, n]: the sum of the absolute values of every term of the distance's formula,
    sum_e ( |1/8 (mu_i - mu_j)^2 / s| + |1/2 ln s| + |lv_i / 4| + |lv_j / 4| ),  s = (e^lv_i + e^lv_j) / 2"""
    enc = np.asarray(enc, dtype=np.float64)
    E = enc.shape[1] // 2
    mu, lv = enc[:, :E], enc[:, E:]
    A = np.zeros((enc.shape[0], enc.shape[0]))
    for e in range(E):   # dimension by dimension: [n, n] temporaries whatever E
        s = 0.5 * (np.exp(lv[:, None, e]) + np.exp(lv[None, :, e]))
        A += 0.125 * (mu[:, None, e] - mu[None, :, e]) ** 2 / s + 0.5 * np.abs(np.log(s))
        A += 0.25 * (np.abs(lv[:, None, e]) + np.abs(lv[None, :, e]))
    return A


def plane_matrices(planes, counts, row0, n_max):
    """what dib_compression_matrices owes on planes [F, plane_rows, 2E]: (dist, comp, A), float64 [F, n_max, n_max] each, zero
    outside [:counts[f], :counts[f]] (counts clamped to [0, n_max])"""
    F = planes.shape[0]
    dist, comp, A = (np.zeros((F, n_max, n_max)) for _ in range(3))
    for f in range(F):
        c = int(min(max(int(counts[f]), 0), n_max))
        rows = planes[f, row0: row0 + c]
        dist[f, :c, :c] = distances(rows)
        comp[f, :c, :c] = np.exp(-dist[f, :c, :c])
        A[f, :c, :c] = magnitude(rows)
    return dist, comp, A


def chain(spec, params, f, x_f):
    """the float64 chain of one feature: encoder, distances, exp(-D) -> (matrix, encodings)"""
    x_f = np.asarray(x_f, dtype=np.float64)
    return orc.compression_matrix(spec, params, f, x_f), orc.encode_feature(spec, params, f, x_f)
