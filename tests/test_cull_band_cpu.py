"""CPU: the cull band (csrc/p3d_cull_band.hpp) against the oracle.  p3d_apply_masks decides the cull / binarize mask from raw
sigma alone outside [s_lo, s_hi] and evaluates the contract's a(s) = 1 - exp_nonpos(-softplus(s - 1)) only inside; this is
bit-identical when, for every float s,  s < s_lo => a(s) < thresh  and  s > s_hi => !(a(s) < thresh).

A host program compiled from the header alone prints the band of each threshold and the header's delta.  a(s) is
oracle.sigma2density(s, None, None).  The sweep, per threshold: every float within 2^21 floats of each band edge; every 2048th bit
pattern of the whole float range (finite values); -1000, +-0, +-inf and the largest and smallest subnormals.  E is the largest
|a(s) - A(s)|, A(s) = 1 / (1 + e^-(s - 1)) in float64, over the whole sweep of all thresholds: the header's delta is 16 E of the
sweep it records, and the test fails when this sweep finds E above delta / 8."""
import subprocess

import numpy as np
import pytest

from host_build import compile_host

THRESHOLDS = [0.5, 0.05, 0.95, 0.999, 1e-3, 1e-7]
WINDOW = 1 << 21


def _ord(f):
    """order-preserving float32 -> int64 (consecutive floats are consecutive integers; -0 and +0 are one apart)"""
    u = np.asarray(f, np.float32).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, -(u & 0x7FFFFFFF) - 1, u)


def _unord(i):
    i = np.asarray(i, np.int64)
    u = np.where(i < 0, (-(i + 1)) | 0x80000000, i)
    return u.astype(np.uint32).view(np.float32)


def _A(s):
    x = s.astype(np.float64) - 1.0
    with np.errstate(over="ignore"):
        e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _whole_range():
    u = np.arange(0, 1 << 32, 2048, dtype=np.uint64).astype(np.uint32)
    s = u.view(np.float32)
    s = s[np.isfinite(s)]
    special = np.array([-1000.0, 0.0, -0.0, np.inf, -np.inf], np.float32)
    sub = np.array([0x007FFFFF, 0x807FFFFF, 0x00000001, 0x80000001], np.uint32).view(np.float32)
    return np.concatenate([s, special, sub])


@pytest.fixture(scope="module")
def bands(tmp_path_factory):
    exe = compile_host(tmp_path_factory.mktemp("cull_band"), "cull_band_host.cpp")
    args = [float(np.float32(t)).hex() for t in THRESHOLDS]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60, check=True).stdout.split("\n")
    res = {}
    for t, line in zip(THRESHOLDS, out):
        th, lo, hi, delta = (float.fromhex(x) if "0x" in x else float(x) for x in line.split())
        assert np.float32(th) == np.float32(t)
        res[t] = (np.float32(lo), np.float32(hi), delta)
    return res


@pytest.fixture(scope="module")
def sweep(bands, oracle):
    """thresh -> (band width in floats, s with a wrong decision below s_lo, ... above s_hi, E of this threshold's sweep)"""
    whole = _whole_range()
    a_whole = oracle.sigma2density(whole, None, None)
    e_whole = float(np.max(np.abs(a_whole.astype(np.float64) - _A(whole))))
    res = {}
    for t, (lo, hi, _) in bands.items():
        th = np.float32(t)
        edges = [e for e in (lo, hi) if np.isfinite(e)]
        idx = np.unique(np.concatenate([np.arange(_ord(e) - WINDOW, _ord(e) + WINDOW + 1) for e in edges]))
        near = _unord(idx)
        assert np.all(np.isfinite(near))
        a_near = oracle.sigma2density(near, None, None)
        s = np.concatenate([near, whole])
        a = np.concatenate([a_near, a_whole])
        bad_lo = s[(s < lo) & ~(a < th)]
        bad_hi = s[(s > hi) & (a < th)]
        e = max(e_whole, float(np.max(np.abs(a_near.astype(np.float64) - _A(near)))))
        width = int(_ord(hi) - _ord(lo)) if len(edges) == 2 else None
        print("thresh %g: s_lo %r s_hi %r, %s floats wide, %d floats swept, E %.3g" % (t, lo, hi, width, s.size, e))
        res[t] = (width, bad_lo, bad_hi, e)
    return res


@pytest.mark.parametrize("thresh", THRESHOLDS)
def test_the_decision_outside_the_band_is_the_contracts(sweep, thresh):
    _, bad_lo, bad_hi, _ = sweep[thresh]
    assert bad_lo.size == 0, "s < s_lo but !(a < thresh): %r" % bad_lo[:8]
    assert bad_hi.size == 0, "s > s_hi but a < thresh: %r" % bad_hi[:8]


def test_the_measured_error_is_within_an_eighth_of_delta(bands, sweep):
    delta = {d for _, _, d in bands.values()}
    assert len(delta) == 1
    delta = delta.pop()
    E = max(e for _, _, _, e in sweep.values())
    print("E %.4g, delta %.4g, delta / 8 %.4g" % (E, delta, delta / 8))
    assert E <= delta / 8


def test_band_widths(bands, sweep):
    for t in THRESHOLDS:
        print("thresh %g: band of %s floats" % (t, sweep[t][0]))
    # at 0.5 the band is about +-50 floats around s = 1 (above 1 a float is 2^-23, below it 2^-24)
    lo, hi, delta = bands[0.5]
    assert lo < np.float32(1.0) < hi and 50 <= sweep[0.5][0] <= 500
    # 1e-7 - delta < 0: the low side is open, so nothing is culled without the full evaluation
    lo, hi, _ = bands[1e-7]
    assert lo == -np.inf and np.isfinite(hi)
