"""CPU: k_render's merge pre-pass by rank search (p3d_merge_ranks_half + p3d_deposit_fine_bits, csrc/p3d_importance.hpp) compiled
for the host with no device code (tests/merge_ranks_host.cpp) and compared word for word — the is-coarse row AND the known row —
with the serial merge of the same header (p3d_merge_bits_half, both halves OR-ed) and with a plain stable two-list merge:

* the shapes the kernels run, (Sc, Sf) = (48, 48), (96, 96), (32, 48), (64, 48), (48, 0), on random lists, fine depths equal to coarse
  ones, a handful of distinct depths, all fine samples in front of all coarse ones and the reverse; every fine sample cropped, none,
  a random quarter;
* every pair of sorted lists of up to 5 + 5 depths over four values: every interleaving, every tie, runs of equal depths on both sides;
* on every shape, i0 coarse samples, k fine ones, the other coarse ones, the other fine ones, for every (i0, k): a coarse and a fine
  sample on every merged position, bits 31, 32, 63 and 64 among them.

The pre-pass's bits decide which samples the walk decodes: a missing known-bit costs a decode and changes no output, so only this
comparison (and the decode-step count of tests/test_hip_merge_ranks.py) pins them."""
import subprocess

import pytest

from host_build import compile_host

SHAPES = [(48, 48), (96, 96), (32, 48), (64, 48), (48, 0)]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = compile_host(tmp_path_factory.mktemp("merge_ranks"), "merge_ranks_host.cpp")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-4000:]
    return dict((l.split()[0], int(l.split()[1])) for l in res.stdout.splitlines())


def test_rank_rows_random_lists(report):
    assert report["random"] == 3000 * len(SHAPES)


def test_rank_rows_every_small_interleaving(report):
    def lists(n):  # sorted lists of n depths over four values
        from math import comb
        return comb(n + 3, 3)
    assert report["small"] == sum(lists(n) for n in range(1, 6)) * sum(lists(n) for n in range(0, 6)) * 3


def test_rank_rows_every_merged_position(report):
    assert report["boundary"] == sum((sc + 1) * (sf + 1) for sc, sf in SHAPES)
    assert report["bits"] > 0  # a coarse and a fine sample on each of the merged positions 31, 32, 63, 64


def test_both_deposits_ran(report):
    """The fine samples' crop bits from their two runs (checked against the bit-by-bit deposit in the host program) and bit by bit."""
    assert report["deposit_runs"] > 10000 and report["deposit_bits"] > 10000
