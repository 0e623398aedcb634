"""GPU: the launch replay of TriPlaneGenerator views (generator.py `_replay_view` / `_capture_view`) against a COLD TWIN — a second
generator built the same way with the same state_dict, replay off, `clear_memo()` before every call, and the same setter calls.
The eager path is pinned to the reference elsewhere (tests/test_hip_synthesis.py, tests/test_dropin_reference.py), so the bar here
is bit-identity: every output of every `G.f` call equals the twin's bit for bit (both sides seeded identically before each call:
the renderer draws its jitter from the device generator even under noise_mode='const').

What is pinned is the replay layer's decision of WHICH launches and WHICH operand buffers a view gets: interleaved call kinds and
subjects that share the prepared conditioning terms, every other eager path that refreshes those terms (sample_mixed, autograd,
cache_backbone, latent injection, stop_level), in-place conditioning writes, the setters and process-wide switches that change the
launches, eviction, seeded random walks over all of it, and the per-subject check of the two-term convolutions' domain.  Every
test also counts the replays that really happened (a test that never replays would pass vacuously).

Setter scenarios assert on the host that no capture survived the switch BEFORE the next call: a capture that outlived
set_conv_mma('f16') / set_sr_mma_f16 would replay launches that read freed operand blocks."""
import random
import warnings

import pytest
import torch

import p3d_shared_cases as MC
import p3d_testing as T

pytestmark = pytest.mark.gpu

KEYS = ("image", "image_raw", "image_depth", "image_weights", "image_xyz", "triplane")


@pytest.fixture(scope="module")
def hip():
    import panic3d_amd
    assert torch.cuda.is_available()
    panic3d_amd._lib.lib()
    return panic3d_amd


def _subject(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return {"image_ortho_front": (torch.rand(1, 3, 32, 32, generator=g) * scale).cuda(), "resnet_feats": torch.randn(1, 16, generator=g).cuda()}


def _x(cond, res=16, nv=1, azim=0.0, noise="const", seed=4, **extra):
    return dict(seeds=[seed], cond=cond, elevations=torch.zeros(nv, device="cuda"),
                azimuths=torch.arange(nv, device="cuda", dtype=torch.float32) * 40.0 + float(azim),
                neural_rendering_resolution=res, noise_mode=noise, triplane_crop=0.1, cull_clouds=0.5, **extra)


class Pair:
    """The generator under test (replay on) and its cold twin."""

    def __init__(self, fill=3):
        self.G = MC.memo_generator("cuda")
        if fill is not None:
            T.fill_generator_params(self.G, fill)
        self.twin = MC.memo_generator("cuda")
        self.twin.load_state_dict(self.G.state_dict())
        self.G.set_view_replay(True)
        self.twin.set_view_replay(False)
        self.calls = 0
        self.total = 0       # replays made on G
        self.evicted = 0     # captures evicted on G

    def both(self, name, *args):
        """The same setter on both generators."""
        for g in (self.G, self.twin):
            getattr(g, name)(*args)

    def entries(self):
        vg = self.G.__dict__.get("_view_graphs")
        return list(vg["entries"].values()) if vg else []

    def no_capture(self):
        return all(e["graph"] is None for e in self.entries())

    def evictions(self):
        vg = self.G.__dict__.get("_view_graphs")
        return vg.get("evictions", 0) if vg else 0

    def _replays(self):
        return {id(e): (e, e.get("replays", 0)) for e in self.entries()}

    def view(self, cond, grad=False, stop_level=None, **kw):
        """One G.f call on both generators (fresh dicts, the same torch seed); asserts bit-identity and returns the number of
        replays the call made on G (0 or 1)."""
        self.calls += 1
        before = self._replays()
        vg0 = self.G.__dict__.get("_view_graphs")
        ev0 = self.evictions()
        outs = []
        for g in (self.G, self.twin):
            if g is self.twin:
                g.clear_memo()
            torch.manual_seed(1000 + self.calls)
            with warnings.catch_warnings():
                if g is self.twin:
                    warnings.simplefilter("ignore")  # (the twin reads the domain flag on every call: its warnings are not the subject)
                with torch.set_grad_enabled(grad):
                    out = g.f(_x(cond, **kw), stop_level=stop_level)
            outs.append({k: out[k].detach().clone() for k in KEYS})
        for k in KEYS:
            a, b = outs[0][k], outs[1][k]
            assert a.dtype == torch.float32 and a.shape == b.shape, (k, a.dtype, a.shape, b.shape)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (self.calls, kw, k, float((a - b).abs().max()))  # bits (NaN too)
        after = self._replays()
        delta = sum(r - before.get(i, (None, 0))[1] for i, (_, r) in after.items())
        self.total += delta
        vg = self.G.__dict__.get("_view_graphs")
        self.evicted += self.evictions() - (ev0 if vg is vg0 else 0)
        self.last = outs[0]
        return delta

    def sample_mixed(self, cond, seed=9):
        """sample_mixed for `cond` on both generators (it refreshes the prepared conditioning terms); same densities / colours."""
        g = torch.Generator().manual_seed(seed)
        coords = (torch.rand(1, 64, 3, generator=g) * 0.5 - 0.25).cuda()
        dirs = torch.nn.functional.normalize(torch.randn(1, 64, 3, generator=g), dim=-1).cuda()
        z = torch.randn(1, 512, generator=g).cuda()
        outs = []
        with torch.no_grad():
            for G in (self.G, self.twin):
                ws = G.mapping(z, torch.zeros(1, 25, device="cuda"), cond)
                outs.append(G.sample_mixed(coords, dirs, ws, cond, noise_mode="const"))
        for k in outs[0]:
            assert torch.equal(outs[0][k], outs[1][k]), k


def _capture(P, cond, **kw):
    """The first call of a kind runs eagerly (on a new generator the one before it too: it reads the domain flag of the new weights),
    the next one is captured and replayed, and the one after that replays."""
    eager = 0
    while P.view(cond, **kw) == 0:
        eager += 1
        assert eager <= 2, "no capture"
    assert P.view(cond, **kw, azim=20.0) == 1


K1 = dict(res=16)


def _other_kind_res(P, B):
    P.view(B, res=24)
    P.view(B, res=24)


def _other_kind_views(P, B):
    P.view(B, nv=2)
    P.view(B, nv=2)


def _sample_mixed(P, B):
    P.sample_mixed(B)


def _grad_call(P, B):
    assert P.view(B, grad=True) == 0


def _cache_backbone(P, B):
    assert P.view(B, cache_backbone=True) == 0
    assert P.view(B, use_cached_backbone=True, azim=30.0) == 0


def _latent_injection(P, B):
    dw = torch.randn(1, P.G.backbone.num_ws, 512, generator=torch.Generator().manual_seed(3)).cuda() * 0.1
    assert P.view(B, latent_injection={"dw": dw}) == 0


def _stop_level(P, B):
    P.view(B, stop_level=1)
    P.view(B, stop_level=1)


@pytest.mark.parametrize("between", [_other_kind_res, _other_kind_views, _sample_mixed, _grad_call, _cache_backbone, _latent_injection,
                                     _stop_level], ids=lambda f: f.__name__.strip("_"))
def test_a_capture_never_replays_terms_prepared_for_another_subject(hip, between):
    """Subject A is captured under kind k1; an eager path prepares the conditioning terms for subject B (another call kind or
    view count, sample_mixed, autograd, cache_backbone, latent injection, stop_level); the next k1 call with A's tensors must see A's
    terms (it runs eagerly and refreshes them), and the one after replays again."""
    P = Pair()
    A, B = _subject(1), _subject(2)
    _capture(P, A, **K1)
    between(P, B)
    P.view(A, **K1)          # the call a stale capture gets wrong
    assert P.view(A, **K1, azim=60.0) == 1
    assert P.view(A, **K1, azim=90.0) == 1


def test_an_in_place_write_to_the_conditioning_is_seen(hip):
    P = Pair()
    A = _subject(1)
    _capture(P, A, **K1)
    assert P.view(A, **K1) == 1
    before = P.last["image"]
    with torch.no_grad():
        A["image_ortho_front"].mul_(0.5)      # the version moves: the next call must see the new values
    assert P.view(A, **K1) == 0
    assert not torch.equal(before, P.last["image"])
    assert P.view(A, **K1) == 1
    A["resnet_feats"].neg_()
    assert P.view(A, **K1) == 0
    assert P.view(A, **K1, azim=45.0) == 1


def test_conv_mma_setters_drop_the_captures(hip):
    """set_conv_mma through x2 -> f32 -> f16 -> x2 -> None, then set_sr_mma_f16(True / False): no capture survives a switch
    (checked before the next call), and every view after a switch equals the twin's under the same switch."""
    P = Pair()
    A = _subject(1)
    _capture(P, A, **K1)
    imgs = {}
    for name, arg in [("set_conv_mma", "x2"), ("set_conv_mma", "f32"), ("set_conv_mma", "f16"), ("set_conv_mma", "x2"),
                      ("set_conv_mma", None), ("set_sr_mma_f16", True), ("set_sr_mma_f16", False)]:
        P.both(name, arg)
        assert P.no_capture(), (name, arg)
        P.view(A, **K1)
        assert P.view(A, **K1, azim=30.0) == 1, (name, arg)
        imgs[(name, arg)] = P.last["image"]
    # the switches really change the launches: f32 / f16 operands are not the two-term ones
    assert not torch.equal(imgs[("set_conv_mma", "f16")], imgs[("set_conv_mma", "x2")])
    assert not torch.equal(imgs[("set_sr_mma_f16", True)], imgs[("set_sr_mma_f16", False)])


def test_noise_pool_switches_are_seen_by_replays(hip):
    """noise_mode='random': G.set_noise_pool(False / True) drops the captures; the process-wide stylegan2.set_noise_pool is part of
    the key (the next call is a new entry, run eagerly)."""
    sg = hip.stylegan2
    P = Pair()
    A = _subject(1)
    kw = dict(K1, noise="random")
    _capture(P, A, **kw)
    for state in (False, True, None):
        P.both("set_noise_pool", state)
        assert P.no_capture(), state
        P.view(A, **kw)
        assert P.view(A, **kw, azim=30.0) == 1, state
    prev = sg.set_noise_pool(not sg.NOISE_POOL)
    try:
        n = len(P.entries())
        assert P.view(A, **kw) == 0 and len(P.entries()) == n + 1   # another entry: the capture under the other noise path is not used
        assert P.view(A, **kw, azim=30.0) == 1
    finally:
        sg.set_noise_pool(prev)
    assert P.view(A, **kw) == 1    # back on the first entry


@pytest.mark.parametrize("setter,values", [("set_render_exact", (False, None, True)), ("set_force_sigmoid", (False, True))])
def test_render_switches_are_keyed(hip, setter, values):
    P = Pair()
    A = _subject(1)
    _capture(P, A, **K1)
    for v in values:
        P.both(setter, v)
        P.view(A, **K1)
        assert P.view(A, **K1, azim=30.0) == 1, v


@pytest.mark.parametrize("switch", ["TORGB_RIDES", "CONV_IMG"])
def test_module_switches_are_keyed(hip, switch, monkeypatch):
    """stylegan2.TORGB_RIDES / CONV_IMG are read at call time and are part of the key (stylegan2.switch_state): flipping one
    makes the next call a new entry instead of replaying the launches of the other setting."""
    sg = hip.stylegan2
    P = Pair()
    A = _subject(1)
    _capture(P, A, **K1)
    key0 = sg.switch_state()
    monkeypatch.setattr(sg, switch, not getattr(sg, switch))
    assert sg.switch_state() != key0
    n = len(P.entries())
    assert P.view(A, **K1) == 0 and len(P.entries()) == n + 1
    assert P.view(A, **K1, azim=30.0) == 1
    monkeypatch.undo()
    assert P.view(A, **K1) == 1


def test_eviction_then_the_first_kind_again(hip):
    P = Pair()
    A = _subject(1)
    kinds = [dict(res=16), dict(res=24), dict(nv=2), dict(res=24, nv=2), dict(nv=3)]
    assert len(kinds) > P.G._REPLAY_MAX
    for k in kinds:
        _capture(P, A, **k)
    assert P.evictions() >= 1 and len(P.entries()) == P.G._REPLAY_MAX
    assert P.view(A, **kinds[0]) == 0          # evicted: eager again
    assert P.view(A, **kinds[0]) == 1
    assert P.view(A, **kinds[-1]) == 1         # the last one is still there
    # captures made before a bigger view replaced the capture stream's convolution workspace (some of their launches use the old
    # one, allocated in an evicted capture's memory pool, and torch.cuda.graph empties the allocator's cache before each capture)
    assert P.view(A, **kinds[2]) == 1 and P.view(A, **kinds[3]) == 1


def test_the_memo_switch_drops_the_captures(hip):
    """Without the memo layer every call re-derives the operands a capture reads (the old ones are freed): a call with it off drops
    the captures, and the first call after it is back on runs eagerly."""
    P = Pair()
    A = _subject(1)
    _capture(P, A, **K1)
    prev = hip.memo.set_enabled(False)
    try:
        assert P.view(A, **K1) == 0 and P.view(A, **K1, azim=30.0) == 0
        assert P.no_capture()
    finally:
        hip.memo.set_enabled(prev)
    assert P.view(A, **K1) == 0
    assert P.view(A, **K1, azim=30.0) == 1


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_seeded_random_walk(hip, seed):
    """~60 steps drawn from call kinds x subjects x noise modes x setters x sample_mixed x in-place conditioning writes x
    load_state_dict; every view equals the twin's bit for bit; the walk replays and evicts."""
    rng = random.Random(seed)
    P = Pair()
    subjects = [_subject(1), _subject(2), _subject(3)]
    kinds = [dict(res=16), dict(res=24), dict(nv=2), dict(res=24, nv=2), dict(nv=3)]
    state = {k: v.clone() for k, v in P.G.state_dict().items()}
    name = "backbone.synthesis.b16.conv1.weight"
    last = (subjects[0], kinds[0], "const")
    for step in range(60):
        r = rng.random()
        if r < 0.40:          # the same call again (mostly a replay), another view
            s, k, nm = last
            P.view(s, noise=nm, azim=rng.choice([0.0, 30.0, 60.0]), **k)
        elif r < 0.70:
            last = (rng.choice(subjects), rng.choice(kinds), rng.choice(["const", "const", "random"]))
            s, k, nm = last
            P.view(s, noise=nm, **k)
        elif r < 0.76:
            P.both("set_conv_mma", rng.choice(["x2", "f32", "f16", None]))
            assert P.no_capture()
        elif r < 0.80:
            P.both("set_sr_mma_f16", rng.random() < 0.5)
            assert P.no_capture()
        elif r < 0.84:
            P.both("set_noise_pool", rng.choice([True, False, None]))
            assert P.no_capture()
        elif r < 0.88:
            P.sample_mixed(rng.choice(subjects), seed=step)
        elif r < 0.93:
            s = rng.choice(subjects)
            with torch.no_grad():
                s["image_ortho_front"].mul_(0.9).add_(0.05)
        elif r < 0.96:
            sd = dict(state, **{name: state[name] * rng.choice([1.0, 1.1])})
            for g in (P.G, P.twin):
                g.load_state_dict(sd)
        else:
            P.both("set_render_exact", rng.choice([True, False, None]))
    assert P.total >= 8, (P.total, P.calls)
    # a closing sweep over more kinds than the generator keeps (the walk's setters drop the captures, so it alone cannot promise one)
    for k in kinds + kinds[:1]:
        P.view(subjects[0], **k)
        P.view(subjects[0], **k)
    assert P.evicted >= 1, P.evicted


def test_the_conv_domain_is_checked_per_subject(hip, monkeypatch):
    """In-domain weights.  Subject A stays silent; subject B's conditioning image is scaled until a two-term layer leaves the domain
    (the twin confirms: its x2 image differs from its f32 image); B's first view warns and sets conv_domain_was_violated; A's views
    afterwards are silent, and the replayed ones do not read the flag."""
    ops = hip.ops
    P = Pair(fill=None)      # the constructor's weights: in the domain for an ordinary subject
    for g in (P.G, P.twin):
        g.set_render_exact(None)
    A = _subject(1)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        _capture(P, A, **K1)
    assert not P.G.__dict__.get("conv_domain_was_violated")

    B = None
    for scale in (1e2, 1e3, 1e4, 1e5, 1e6):      # the smallest scale that saturates (the twin reads its flag on every call)
        cand = _subject(2, scale)
        P.twin.__dict__["conv_domain_was_violated"] = False
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            P.twin.clear_memo()
            with torch.no_grad():
                P.twin.f(_x(cand, **K1))
        if P.twin.__dict__.get("conv_domain_was_violated"):
            B = cand
            break
    assert B is not None, "no scale of the conditioning image left the two-term domain"
    outs = {}
    for mode in ("f32", "x2"):
        P.twin.set_conv_mma(mode)
        P.twin.clear_memo()
        with warnings.catch_warnings(), torch.no_grad():
            warnings.simplefilter("ignore")
            outs[mode] = P.twin.f(_x(B, **K1))["image"].clone()
    P.twin.set_conv_mma(None)
    diff = float((outs["x2"] - outs["f32"]).abs().nan_to_num(nan=float("inf")).max())
    assert not torch.equal(outs["x2"], outs["f32"]) and diff > 1e-3 * max(1.0, float(outs["f32"].abs().max())), diff   # it really saturates

    reads = []
    real = ops.conv_domain_violated

    def counted(word, reset=True):
        if any(word is w for w in P.G.__dict__["_conv_domain_flag"].words.values()):
            reads.append(1)
        return real(word, reset)
    monkeypatch.setattr(ops, "conv_domain_violated", counted)

    with pytest.warns(RuntimeWarning, match="saturated"):
        assert P.view(B, **K1) == 0
    assert P.G.__dict__.get("conv_domain_was_violated") and len(reads) == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        assert P.view(A, **K1) == 0                  # a subject change: eager, one read, in the domain
        assert len(reads) == 2
        for az in (30.0, 60.0, 90.0):
            assert P.view(A, **K1, azim=az) == 1     # replays: silent, no read
    assert len(reads) == 2
