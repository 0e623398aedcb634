"""CPU: k_render's tile order (p3d_tile_of_block / p3d_tile_screen, csrc/p3d_render_plan.hpp), evaluated by a host program
compiled from the header the kernel includes (tests/tile_order_host.cpp).  For every shape and workgroup size: the map
block -> (tile, wave) is a bijection onto [0, ntiles) plus padding, the tiles cover every view's screen exactly once, and a
workgroup never straddles two runs.  Where the plan takes the balanced pieces (pw x ph tiles, the piece of column c and row r
dealt to XCD (a * c + r + s * (r // 8)) % 8): every block of XCD b % 8 lies in a piece the rule gives that XCD, every XCD gets
the same number of pieces, visits every piece column, and gets as many piece rows from the inner half of the view as from the outer half.  Shapes that do not divide keep the
round-5 order, and a map with two XCDs swapped for one piece row fails the same assertions."""
import subprocess

import numpy as np
import pytest

from host_build import compile_host

NO_PAIR = 256
# name -> (views, width, height, flags, takes the piece order)
SHAPES = {
    "512^2": (1, 512, 512, 0, True),
    "256^2": (1, 256, 256, 0, True),
    "4 x 256^2": (4, 256, 256, 0, True),
    "1024^2": (1, 1024, 1024, 0, True),
    "128 x 512": (1, 128, 512, 0, True),
    "384^2": (1, 384, 384, 0, False),             # 18 super-tiles, 24 piece rows in 3 columns
    "2 x 384 x 256": (2, 384, 256, 0, True),      # 3 piece columns
    "8 x 128^2": (8, 128, 128, 0, False),         # 8 piece rows in one column: an XCD's row is inner or outer, not both
    "128^2": (1, 128, 128, NO_PAIR, False),       # 2 super-tiles: fewer than 8 of the pieces any order deals
}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return compile_host(tmp_path_factory.mktemp("tile_order"), "tile_order_host.cpp")


def tile_map(exe, N, W, H, flags, nw=0, parent=0, rule=(0, 0, 0, 0)):
    req = f"m {N} {W * H} {W} 48 48 {flags} {nw} {parent} {rule[0]} {rule[1]} {rule[2]} {rule[3]}\n"
    out = subprocess.run([exe], input=req, capture_output=True, text=True, timeout=120, check=True).stdout.splitlines()
    h = out[0].split()
    assert h[0] == "order", out[0]
    head = dict(zip(("swz", "blocked", "pieces", "pw", "ph", "xa", "xs", "nwaves", "grid", "tiles_x", "tiles_per_img", "ntiles"), map(int, h[1:])))
    m = np.array([[int(v) for v in l.split()] for l in out[1:]], dtype=np.int64)
    return head, dict(zip(("block", "wave", "tile", "view", "tx", "ty"), m.T))


def check_map(head, m, N, W, H):
    """Every property that holds under every order."""
    nw, grid, ntiles = head["nwaves"], head["grid"], head["ntiles"]
    assert ntiles == N * (W // 8) * (H // 4) and grid == -(-ntiles // nw)
    assert len(m["tile"]) == grid * nw
    assert np.array_equal(np.sort(m["tile"]), np.arange(grid * nw)), "block -> (tile, wave) is not a bijection"
    real = m["tile"] < ntiles
    assert real.sum() == ntiles and np.all(m["view"][~real] == -1)
    screen = (m["view"][real] * (H // 4) + m["ty"][real]) * (W // 8) + m["tx"][real]
    assert np.all((m["tx"][real] >= 0) & (m["tx"][real] < W // 8) & (m["ty"][real] >= 0) & (m["ty"][real] < H // 4))
    assert np.array_equal(np.sort(screen), np.arange(ntiles)), "the tiles do not cover every screen exactly once"
    # the waves of a workgroup render consecutive tiles of one view
    t = m["tile"].reshape(grid, nw)
    assert np.all(t[:, 1:] == t[:, :-1] + 1) and np.all(t[:, 0] % nw == 0)


def check_pieces(head, m, N, W, H):
    """What the piece order promises on top (the plan took it)."""
    PW, PH, xa, xs, nw = head["pw"], head["ph"], head["xa"], head["xs"], head["nwaves"]
    assert head["pieces"] == 1 and PW * PH < 256 and (W // 8) % PW == 0 and (H // 4) % PH == 0
    PC, PR = W // 8 // PW, H // 4 // PH
    assert head["swz"] * nw == PW * PH and head["ntiles"] % (PW * PH) == 0
    assert np.all(m["tile"] < head["ntiles"])  # whole pieces: no padding
    x, c, r = m["block"] % 8, m["tx"] // PW, m["ty"] // PH
    assert np.array_equal(x, (xa * c + r + xs * (r // 8)) % 8), "a block lies in a piece the rule gives another XCD"
    piece = (m["view"] * PR + r) * PC + c
    assert np.all(piece.reshape(head["grid"], nw) == piece.reshape(head["grid"], nw)[:, :1]), "a workgroup straddles two pieces"
    inner = (r >= PR // 4) & (r < PR - PR // 4)
    per_xcd = []
    for k in range(8):
        own = np.unique(piece[x == k])
        per_xcd.append(len(own))
        assert set((own % PC).tolist()) == set(range(PC)), f"XCD {k} does not visit every piece column"
        rows_in = len(np.unique(piece[(x == k) & inner]))
        assert 2 * rows_in == len(own), f"XCD {k}: {rows_in} of its {len(own)} pieces lie in the inner half of the rows"
        # an XCD works through one piece after the other: its blocks, in dispatch order, change piece every swz blocks
        seq = piece.reshape(head["grid"], nw)[k::8, 0]
        assert np.all(seq.reshape(-1, head["swz"]) == seq.reshape(-1, head["swz"])[:, :1])
    assert len(set(per_xcd)) == 1 and per_xcd[0] * 8 == N * PC * PR, per_xcd


@pytest.mark.parametrize("nw", [1, 2, 4])
@pytest.mark.parametrize("name", list(SHAPES))
def test_tile_order(host, name, nw):
    N, W, H, flags, pieces = SHAPES[name]
    head, m = tile_map(host, N, W, H, flags, nw)
    assert head["nwaves"] == nw
    check_map(head, m, N, W, H)
    parent_head, parent = tile_map(host, N, W, H, flags, nw, parent=1)
    assert parent_head["pieces"] == 0
    check_map(parent_head, parent, N, W, H)
    if pieces:
        check_pieces(head, m, N, W, H)
    else:
        # the fallback IS the round-5 order
        assert head == parent_head and all(np.array_equal(m[k], parent[k]) for k in m)


def test_the_plans_own_workgroup_size(host):
    for name, (N, W, H, flags, pieces) in SHAPES.items():
        head, m = tile_map(host, N, W, H, flags)
        check_map(head, m, N, W, H)
        assert head["pieces"] == int(pieces), name
        if pieces:
            check_pieces(head, m, N, W, H)


def test_parent_order_hands_each_xcd_whole_super_tiles(host):
    head, m = tile_map(host, 1, 512, 512, 0, parent=1)
    assert (head["blocked"], head["pieces"], head["swz"] * head["nwaves"]) == (1, 0, 256)
    st = (m["ty"] // 16) * 4 + m["tx"] // 16
    for k in range(8):
        own = np.unique(st[m["block"] % 8 == k])
        assert len(own) == 4 and set((own % 4).tolist()) == {0, 1, 2, 3}


def test_a_wrong_rule_is_caught(host):
    # seeded fault: two XCDs swapped for piece row 3 (their blocks exchanged): the map stays a bijection, the rule check fails
    N, W, H, flags, _ = SHAPES["512^2"]
    head, m = tile_map(host, N, W, H, flags)
    check_pieces(head, m, N, W, H)
    bad = dict(m)
    row3 = m["ty"] // head["ph"] == 3
    x = m["block"] % 8
    xp, xq = np.unique(x[row3])[:2]  # two XCDs that own a piece of that row
    ip, iq = np.flatnonzero(row3 & (x == xp)), np.flatnonzero(row3 & (x == xq))
    assert len(ip) == len(iq) > 0  # as many pieces each
    bad["block"] = m["block"].copy()
    bad["block"][ip], bad["block"][iq] = m["block"][iq], m["block"][ip]
    assert np.array_equal(np.sort(bad["block"]), np.sort(m["block"])) and not np.array_equal(bad["block"], m["block"])
    with pytest.raises(AssertionError):
        check_pieces(head, bad, N, W, H)
    # ... and so is another rule's map held against the plan's rule
    other_head, other = tile_map(host, N, W, H, flags, rule=(head["pw"], head["ph"], (head["xa"] + 2) % 8, head["xs"]))
    check_map(other_head, other, N, W, H)
    with pytest.raises(AssertionError):
        check_pieces(head, other, N, W, H)
