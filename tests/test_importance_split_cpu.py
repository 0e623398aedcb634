"""CPU: the schedules that share k_render's per-ray importance work between the two halves of a wave (csrc/p3d_importance.hpp),
compiled for the host with no device code and proved there (tests/importance_split_host.cpp):

* the half sort — every one of the 2^24 zero-one inputs of the 24-key network, and for the 24- and 48-key networks every merge
  pass on every pair of sorted zero-one blocks it has to merge (by induction over the passes the network sorts);
* the cross-half exchange followed by the local merge — every pair of sorted zero-one halves, (Sf/2 + 1)^2 cases, Sf = 48, 96;
* the whole split sort on random and tie-heavy floats against std::sort, bit for bit;
* the split merge pre-pass against a plain stable two-list merge (coarse first on ties) on random and tie-heavy lists — fine
  depths equal to coarse ones, repeated depths, disjoint ranges, ragged and empty lists — both bit rows word for word."""
import subprocess

import pytest

from host_build import compile_host


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = compile_host(tmp_path_factory.mktemp("importance_split"), "importance_split_host.cpp")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-4000:]
    return dict((l.split()[0], int(l.split()[1])) for l in res.stdout.splitlines())


def test_half_sort_all_zero_one_inputs(report):
    assert report["sort24"] == 1 << 24


def test_half_sort_merge_passes(report):
    # blocks of pp keys against their neighbours, (n1 + 1) * (n2 + 1) contents each
    def cases(H):
        n, pp = 0, 1
        while pp < H:
            n += sum((min(pp, H - b) + 1) * (max(0, min(pp, H - b - pp)) + 1) for b in range(0, H, 2 * pp))
            pp *= 2
        return n
    assert report["passes24"] == cases(24) and report["passes48"] == cases(48)


def test_cross_half_merge_all_sorted_zero_one_halves(report):
    assert report["cross24"] == 25 * 25 and report["cross48"] == 49 * 49


def test_split_sort_floats(report):
    assert report["floats24"] == 20000 and report["floats48"] == 20000


def test_split_merge_bit_rows(report):
    assert report["merge"] == 10 * 4000
