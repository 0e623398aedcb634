"""GPU (-m gpu): CLIP's image tower and the 2-D metrics on the HIP kernels (include/p3d_clip.h, panic3d_amd/clip.py, metrics.psnr).  Stage
level: every kernel on the binary32 inputs of the float64 restatement (tests/clip_cases.py).  The GEMM per value within
8 sqrt(K) 2^-24 sum|terms| (the products, the bias, the residual; QuickGELU carried through as clip_cases' docstring derives) and rel-L2
<= 1e-5, for every epilogue under EVERY plan (both tiles; no split, two, as many as there are chunks), two runs the same bits; LayerNorm
and attention: error against float64 at most 4 x that of torch's binary32 F.layer_norm / softmax attention on the same inputs on the CPU,
in max-abs and in rel-L2, per case; the front end's integers equal to Pillow's resize + crop and the normalisation within 2 2^-24 |value|.
Whole network: embedding rel-L2 against float64 <= 4 x torch binary32's on the CPU; the one-call walk gives the bits of the step-by-step
operators.  The gates' sensitivity to seeded faults is shown on CPU in tests/test_clip_cpu.py.  On the parent commit the module, the
operators and the symbols do not exist."""
import ctypes

import pytest
import torch

import clip_cases as CC

pytestmark = pytest.mark.gpu
F = torch.nn.functional


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    panic3d_amd._lib.lib()
    return panic3d_amd


# ---- the GEMM -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CC.GEMM_SHAPES)
def test_gemm_every_epilogue_under_every_plan(P, shape):
    c = CC.gemm_case(shape)
    M, K, Nout = shape
    bad, seen = [], set()
    for plan in CC.PLANS:
        pl = P.ops.clip_gemm_plan(M, K, Nout, plan)
        seen.add((pl["tile"], pl["split"]))
        for bias, gelu, res in CC.EPILOGUES:
            y, s, terms = CC.gemm_ref(c, bias, gelu, res)
            a, b = CC.run_gemm(P.ops, c, bias, gelu, res, "cuda", plan), CC.run_gemm(P.ops, c, bias, gelu, res, "cuda", plan)
            assert torch.equal(a, b), f"two runs differ under plan {plan:#x}"
            bad += CC.gate(f"gemm {shape} plan {plan:#x} (tile {pl['tile']}, split {pl['split']}) bias {bias} gelu {gelu} res {res}", a.cpu(), y, s, terms,
                           verbose=(plan == 0))
    assert bad == []
    assert {t for t, _ in seen} == {1, 2}
    if K > 64:
        assert max(s for _, s in seen) == -(-K // 64) and (1, 1) in seen and (2, 1) in seen  # the splits were real ones
    # the residual written in place: out == res
    r = c["res"].cuda()
    keep = r.clone()
    y = P.ops.clip_gemm(c["a"].cuda(), c["w"].cuda(), c["bias"].cuda(), r, inplace=True)
    assert y.data_ptr() == r.data_ptr() and torch.equal(y, P.ops.clip_gemm(c["a"].cuda(), c["w"].cuda(), c["bias"].cuda(), keep))


@pytest.mark.parametrize("case", CC.PATCH_CASES)
def test_patch_mode_against_float64_conv2d(P, case):
    c = CC.patch_case(*case)
    bad = []
    for plan in CC.PLANS:
        a = P.ops.clip_gemm(c["x"].cuda(), c["wk"].cuda(), patch=c["patch"], force_plan=plan)
        assert torch.equal(a, P.ops.clip_gemm(c["x"].cuda(), c["wk"].cuda(), patch=c["patch"], force_plan=plan))
        bad += CC.gate(f"patch {case} plan {plan:#x}", a.cpu(), c["y"], c["y_abs"], c["K"], verbose=(plan == 0))
    assert bad == []


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", CC.LN_D)
def test_layernorm_against_torchs_binary32_error(P, D):
    bad = []
    for M in CC.LN_M:
        for kind in ("plain", "offset"):
            c = CC.ln_case(M, D, kind)
            y = P.ops.clip_layernorm(c["x"].cuda(), c["gamma"].cuda(), c["beta"].cuda())
            assert torch.equal(y, P.ops.clip_layernorm(c["x"].cuda(), c["gamma"].cuda(), c["beta"].cuda())), "two runs differ"
            bad += CC.ln_gate(f"{kind} M={M} D={D}", y, c)
        k = CC.ln_case(M, D, "constant")
        y = P.ops.clip_layernorm(k["x"].cuda(), k["gamma"].cuda(), k["beta"].cuda())
        assert torch.equal(y.cpu(), k["beta"].expand(M, D)), "a constant row must give beta"
    assert bad == []


def test_layernorm_strided_class_token_and_embedding_forms(P):
    g = torch.Generator().manual_seed(2)
    bad = []
    for N, T, D in ((3, 5, 128), (1, 10, 192), (2, 50, 768), (2, 1, 64)):
        c = CC.ln_case(N * T, D)
        x = c["x"].cuda()
        # ln_post: the class token of each image, rows N apart T * D floats
        y = P.ops.clip_layernorm(x, c["gamma"].cuda(), c["beta"].cuda(), rows=N, ld=T * D)
        rows = dict(c, x=c["x"].view(N, T, D)[:, 0].contiguous())
        assert tuple(y.shape) == (N, D) and torch.equal(y, P.ops.clip_layernorm(rows["x"].cuda(), c["gamma"].cuda(), c["beta"].cuda()))
        bad += CC.ln_gate(f"class token N={N} T={T} D={D}", y, rows)
        if T > 1:
            patches, cls, pos = torch.randn(N * (T - 1), D, generator=g), torch.randn(D, generator=g), torch.randn(T, D, generator=g) * 0.5
            e = P.ops.clip_embed(patches.cuda(), cls.cuda(), pos.cuda(), c["gamma"].cuda(), c["beta"].cuda())
            assert torch.equal(e, P.ops.clip_embed(patches.cuda(), cls.cuda(), pos.cuda(), c["gamma"].cuda(), c["beta"].cuda()))
            x32 = (torch.cat([cls.expand(N, 1, D), patches.reshape(N, T - 1, D)], 1) + pos).reshape(N * T, D)  # (one binary32 addition: exact to restate)
            bad += CC.ln_gate(f"embed N={N} T={T} D={D}", e, c, x=x32)
    assert bad == []


# ---- attention ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", CC.ATTN_T)
def test_attention_against_torchs_binary32_error(P, T):
    bad = []
    for heads in CC.ATTN_HEADS:
        for N in CC.ATTN_N:
            c = CC.attn_case(N, T, heads)
            y = P.ops.clip_attention(c["qkv"].cuda(), N, T, heads)
            assert torch.equal(y, P.ops.clip_attention(c["qkv"].cuda(), N, T, heads)), "two runs differ"
            bad += CC.attn_gate(f"N={N} T={T} heads={heads}", y, c)
    assert bad == []


@pytest.mark.parametrize("kind", ["pm80", "pm120", "dominant"])
def test_attention_extreme_logits(P, kind):
    bad = []
    for N, T, heads in ((3, 17, 3), (1, 50, 1)):
        c = CC.attn_case(N, T, heads, kind)
        y = P.ops.clip_attention(c["qkv"].cuda(), N, T, heads)
        assert torch.isfinite(y).all()
        bad += CC.attn_gate(f"{kind} N={N} T={T} heads={heads}", y, c)
    assert bad == []


def test_attention_refuses_what_it_cannot_do(P):
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(ValueError, match="at most 64"):
        P.ops.clip_attention(z(65, 192), 1, 65, 1)
    with pytest.raises(ValueError, match="64 \\* heads"):
        P.ops.clip_attention(z(10, 3 * 100), 2, 5, 2)
    L = P._lib.lib()
    q, o = z(65, 192), z(65, 64)
    assert L.p3d_clip_attention_f32(q.data_ptr(), 1, 65, 1, 64, o.data_ptr(), None) == -2   # T = 65
    assert L.p3d_clip_attention_f32(q.data_ptr(), 1, 5, 2, 100, o.data_ptr(), None) == -2   # D != 64 heads
    with pytest.raises(ValueError):
        P.ops.clip_gemm(z(4, 8), z(9, 3))
    with pytest.raises(ValueError):
        P.ops.clip_gemm(z(4, 8), z(8, 3), z(4))
    with pytest.raises(ValueError):
        P.ops.clip_gemm(z(1, 3, 64, 64), z(3 * 32 * 32, 8), patch=24)
    with pytest.raises(RuntimeError):
        P.ops.clip_gemm(z(4, 8), z(8, 3), force_plan=3 << 8 | 1)
    with pytest.raises(ValueError):
        P.ops.clip_layernorm(z(4, 8), z(8), z(8), rows=3, ld=16)
    with pytest.raises(ValueError):
        P.ops.clip_prepare(z(1, 2, 8, 8), 4)


# ---- the front end --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,S", CC.RESIZE_CASES)
def test_front_end_is_pillows_bit_for_bit(P, hw, S):
    pytest.importorskip("PIL")
    img = CC.image_case(hw, channels=4)  # multiples of 1 / 255; the fourth channel is ignored
    y = P.ops.clip_prepare(img.cuda(), S)
    assert torch.equal(y, P.ops.clip_prepare(img.cuda(), S)), "two runs differ"
    assert CC.prepare_gate(f"{hw}->{S}", y.cpu(), img, S) == []


def test_front_end_clamps_and_floors_arbitrary_floats(P):
    pytest.importorskip("PIL")
    img = CC.image_case((301, 187), levels=False, batch=2)  # floats in [-0.2, 1.2]
    assert float(img.min()) < -0.1 and float(img.max()) > 1.1
    assert CC.prepare_gate("floats (301, 187)->224", P.ops.clip_prepare(img.cuda(), 224).cpu(), img, 224) == []


# ---- the whole network ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CC.NETWORK_CASES))
def test_whole_network(P, name):
    c = CC.network_case(name)
    model = P.CLIPVisual(**c["arch"])
    model.load_state_dict(c["sd"])
    model.cuda()
    img = c["img"].cuda()
    fused = model(img)
    assert torch.isfinite(fused).all() and CC.network_gate(name, fused, c) == []
    assert torch.equal(fused, model(img, fused=False)), "the table walk and the step-by-step operators differ"
    assert torch.equal(fused, model(img)), "two runs differ"
    x = c["x"].cuda()
    assert torch.equal(model.encode_image(x), fused) and torch.equal(model.encode_image(x, fused=False), fused)
    if name == "full":
        assert tuple(fused.shape) == (2, 512)
        assert model.program(2)[0].launches == 138  # 88 steps + the 50 GEMMs' split-K reductions


def test_walk_refuses_bad_records_before_any_launch(P):
    """Bad buffer index, short buffer, workspace too small: each is refused, and the arena is untouched afterwards."""
    c = CC.network_case("tiny1")
    model = P.CLIPVisual(**c["arch"])
    model.load_state_dict(c["sd"])
    model.cuda()
    recs, buf_len, _ = model.records(3, None, plan=1 << 8 | 2)
    blob, _ = model.operands()
    L = P._lib.lib()

    def run(recs, buf_len=buf_len, ws_bytes=None):
        prog = P.ops.ClipProgram(recs, buf_len, blob)
        prog.arena.fill_(7.0)
        need = L.p3d_clip_workspace_bytes(prog.table, len(recs))
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
        rc = L.p3d_clip_forward_f32(prog.table, len(recs), blob.data_ptr(), blob.numel(), prog.arena.data_ptr(), prog.arena.numel(), prog.buf_off, prog.buf_len,
                                    prog.n_bufs, ws.data_ptr(), need if ws_bytes is None else ws_bytes, None)
        torch.cuda.synchronize()
        return rc, prog, need
    rc, prog, need = run(recs)
    assert rc == 0 and need > 0 and not bool((prog.buffer(8, (3, 32)) == 7.0).any())
    last = len(recs) - 1
    for fault in (dict(src=9), dict(dst=-1), dict(res=12)):
        rc, prog, _ = run(recs[:last] + [dict(recs[last], **fault)])
        assert rc == -2 and bool((prog.arena == 7.0).all()), fault
    short = list(buf_len)
    short[8] -= 1
    rc, prog, _ = run(recs, buf_len=short)
    assert rc == -2 and bool((prog.arena == 7.0).all())
    rc, prog, _ = run(recs, ws_bytes=need - 1)
    assert rc == -3 and bool((prog.arena == 7.0).all())


# ---- the similarity -------------------------------------------------------------------------------------------------------------------
def test_similarity_against_float64(P):
    c = CC.network_case("tiny1")
    model = P.CLIPVisual(**c["arch"])
    model.load_state_dict(c["sd"])
    sim = P.CLIPSimilarity(model.cuda())
    a = c["img"]
    b = (a + 0.1 * torch.randn(a.shape, generator=torch.Generator().manual_seed(9))).clamp(0, 1)
    eb64, eb32 = (CC.network(c["sd"], CC.preprocess(b, 64), 2, dt) for dt in (torch.float64, torch.float32))
    want, torch32 = CC.cosine(c["f64"], eb64), CC.cosine(c["f32"], eb32)
    s = sim(a.cuda(), b.cuda())
    e, e32 = float((s.double().cpu() - want).abs().max()), float((torch32.double() - want).abs().max())
    print(f"clip similarity: {s.tolist()}, abs error ours {e:.3e}, torch32 {e32:.3e}")
    assert tuple(s.shape) == (3,) and e <= 4 * e32
    same = sim(a.cuda(), a.cuda())
    assert float((same - 1).abs().max()) <= 4 * 2.0 ** -24
    assert torch.equal(sim(b.cuda(), a.cuda()), s), "the similarity must be symmetric to the bit"
    assert torch.equal(sim(a.cuda(), b.cuda()), s), "two runs differ"
    with pytest.raises(NotImplementedError, match="inference only"):
        sim(a.cuda().requires_grad_(True), b.cuda())


# ---- PSNR -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CC.PSNR_SHAPES)
def test_psnr_against_float64(P, shape):
    c = CC.psnr_case(shape)
    p, t = c["pred"].cuda(), c["target"].cuda()
    for rng in (None, 1.0):
        got, want = P.psnr(p, t, rng), CC.psnr64(c["pred"], c["target"], rng)
        print(f"psnr {shape} data_range {rng}: {got:.9f} dB, float64 {want:.9f} dB")
        assert abs(got - want) <= 1e-5 * abs(want)
        assert P.psnr(p, t, rng) == got, "two runs differ"
    sums = P.ops.psnr_sums(p, t).cpu()
    assert float(sums[1]) == float(c["target"].min()) and float(sums[2]) == float(c["target"].max())
    assert P.psnr(t, t) == float("inf")
    const = torch.full(shape, 0.5, device="cuda")
    import math
    assert P.psnr(p, const) == float("-inf") and math.isnan(P.psnr(const, const))  # range 0: the formula as torch evaluates it


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_image_metrics_on_a_rendered_view(P):
    """image_metrics on a rendered G.f view against a shifted copy: all three keys are finite and clip < 1."""
    import p3d_shared_cases as SC
    G = SC.memo_generator("cuda")
    g = torch.Generator().manual_seed(2)
    cond = {"image_ortho_front": torch.rand(1, 3, 32, 32, generator=g).cuda(), "resnet_feats": torch.randn(1, 16, generator=g).cuda()}
    view = ((SC.memo_call(G, cond, "cuda") + 1) / 2).clamp(0, 1).contiguous()
    assert tuple(view.shape) == (1, 3, 512, 512) and float(view.std()) > 0
    c = CC.network_case("tiny1")
    model = P.CLIPVisual(**c["arch"])
    model.load_state_dict(c["sd"])
    m = P.image_metrics(view, view.roll(16, -1).contiguous(), P.LPIPSLoss().cuda(), P.CLIPSimilarity(model.cuda()))
    print("image_metrics on a rendered view against a copy shifted by 16 pixels:", m)
    assert set(m) == {"lpips", "psnr", "clip"} and all(isinstance(v, float) and v == v and abs(v) < float("inf") for v in m.values())
    assert m["clip"] < 1.0 and m["lpips"] > 0.0
    same = P.image_metrics(view, view.clone(), P.LPIPSLoss().cuda(), P.CLIPSimilarity(model))
    assert same["psnr"] == float("inf") and abs(same["clip"] - 1.0) <= 4 * 2.0 ** -24 and abs(same["lpips"]) <= 1e-6
