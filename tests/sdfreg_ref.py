"""float64 restatement of sdf_bce_reg_loss (reference model/geometry/dmtet.py:161-169) with an explicit loop over the edge rows: the
yardstick of tests/test_sdfreg_cpu.py and tests/test_sdfreg_gpu.py.

    (a, b) = (sdf[e0], sdf[e1]);  the row crosses iff sign3(a) != sign3(b),  sign3(x) = (x > 0) - (x < 0): -0.0, 0.0 and a NaN are 0
    bce(x, t) = max(x, 0) - x t + log1p(exp(-|x|))
    loss = sum bce(a, [b > 0]) / M + sum bce(b, [a > 0]) / M over the M crossing rows (M == 0: nan)
    g_sdf[e0] += (sigmoid(a) - [b > 0]) / M,  g_sdf[e1] += (sigmoid(b) - [a > 0]) / M  (M == 0: zeros)

Python floats are doubles.  Written for finite values; which class (nan, +inf, -inf, finite) a non-finite input lands in is taken from
the float32 torch statements, not from here.
"""
import math

import torch


def sign3(x):
    return (x > 0) - (x < 0)


def bce(x, t):
    return max(x, 0.0) - x * t + math.log1p(math.exp(-abs(x)))


def sigmoid(x):
    if x >= 0:
        return 1.0 / (1.0 + math.exp(-x))
    e = math.exp(x)
    return e / (1.0 + e)


def sdf_bce_reg_loss(sdf, all_edges):
    """-> (loss float, gradient float64 [Nv] for g = 1, crossing mask bool [Ne])"""
    val = [float(v) for v in sdf.reshape(-1).double().tolist()]
    rows = all_edges.tolist()
    mask = [sign3(val[e0]) != sign3(val[e1]) for e0, e1 in rows]
    m = sum(mask)
    sum_a = sum_b = 0.0
    grad = [0.0] * len(val)
    for (e0, e1), crossing in zip(rows, mask):
        if not crossing:
            continue
        a, b = val[e0], val[e1]
        ta, tb = float(b > 0), float(a > 0)
        sum_a += bce(a, ta)
        sum_b += bce(b, tb)
        grad[e0] += (sigmoid(a) - ta) / m
        grad[e1] += (sigmoid(b) - tb) / m
    loss = sum_a / m + sum_b / m if m else float("nan")
    return loss, torch.tensor(grad, dtype=torch.float64), torch.tensor(mask, dtype=torch.bool)
