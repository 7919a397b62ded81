"""tests/psd_scaling_reference.py `skron_error` for sides where its arrays no longer fit: the same exact integer arithmetic on the packed
upper triangle of W (x)_s W, W = R R' at 50 digits, evaluated over slices of whole columns of the block.  W as integers and its float64
scale are computed once; per slice only the (i, j, k, l) of its entries and their products exist, so memory is bounded by the slice
(side 128: 34 million packed entries, about 1.5 million at a time).  Same expressions, same units (eps x skron(|R| |R|')), same result:
tests/test_psd_scaling_large_reference.py holds the two to `==` at sides where both run."""
import math

import numpy as np

from tests import psd_scaling_reference as sr
from tests import psd_step_reference as pr

SLICE_ENTRIES = 1_500_000


def _column_slices(numel, limit):
    """[(b0, b1)]: runs of whole columns b0 .. b1 - 1 of the packed block (column b has b + 1 entries), at most `limit` entries each
    (a single column may exceed it)"""
    out, b0, count = [], 0, 0
    for b in range(numel):
        if count and count + b + 1 > limit:
            out.append((b0, b))
            b0, count = b, 0
        count += b + 1
    out.append((b0, numel))
    return out


def skron_error(R, block, limit=SLICE_ENTRIES):
    """-> the error of `block` (packed upper triangle, column-major, of a float64 W (x)_s W) against skron of the exact R R', in units of
    eps x skron(|R| |R|'): the value of psd_scaling_reference.skron_error"""
    n = R.shape[0]
    Wi, e = pr._ints(pr.mm(pr.M(R), pr.M(R).T))                             # once: W = Wi 2^e
    Wa = np.abs(R) @ np.abs(R).T
    r, c = pr._idx(n)
    numel = len(r)
    block = np.asarray(block, dtype=np.float64)
    assert block.size == numel * (numel + 1) // 2
    s2 = sr.mpf(math.sqrt(2.0))
    s2i, s2e = int(s2.man), int(s2.exp)
    sc2 = math.sqrt(2.0)
    worst = 0.0
    for b0, b1 in _column_slices(numel, limit):
        lo, hi = b0 * (b0 + 1) // 2, b1 * (b1 + 1) // 2
        cols = np.repeat(np.arange(b0, b1), np.arange(b0 + 1, b1 + 1))
        rows = np.arange(lo, hi) - (cols * (cols + 1)) // 2
        i, j, k, l = r[rows], c[rows], r[cols], c[cols]
        v = block[lo:hi]
        ij, kl = i == j, k == l
        err, scale = np.zeros(hi - lo), np.zeros(hi - lo)
        # the four cases of skron!, as in psd_scaling_reference.skron_error
        for m, a, b, c2, d2, root in ((~ij & ~kl, (i, k), (j, l), (i, l), (j, k), False), (ij & ~kl, (j, l), (j, k), None, None, True),
                                      (~ij & kl, (i, l), (j, k), None, None, True), (ij & kl, (j, l), (j, l), None, None, False)):
            if not m.any():
                continue
            ref = Wi[a[0][m], a[1][m]] * Wi[b[0][m], b[1][m]]
            sc = Wa[a[0][m], a[1][m]] * Wa[b[0][m], b[1][m]]
            if c2 is not None:
                ref = ref + Wi[c2[0][m], c2[1][m]] * Wi[d2[0][m], d2[1][m]]
                sc = sc + Wa[c2[0][m], c2[1][m]] * Wa[d2[0][m], d2[1][m]]
            if root:
                ref, sc = ref * s2i, sc2 * sc
            err[m] = sr._exact_error(v[m], ref, 2 * e + (s2e if root else 0))
            scale[m] = sc
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(scale > 0, err / (sr.EPS * scale), np.where(err > 0, np.inf, 0.0))
        worst = max(worst, float(np.max(q)))
    return worst
