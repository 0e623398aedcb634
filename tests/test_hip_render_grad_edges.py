"""GPU: the renderer / point-decode backward kernels (include/p3d_render_grad.h) on the designed edge matrix of
tests/render_grad_cases.py against the float64 restatements of tests/render_grad_ref.py: relative L2 per tensor, exact zeros
outside the touched map, finiteness; then the header's output contract through the C ABI.  Mask decisions come from the library's
own forward (ops.triplane_decode at the binary32 sample points); tests/test_render_grad_ref_cpu.py shows that the gate is
trustworthy (conditioning) and tight (mutations)."""
import ctypes as C

import pytest
import torch

import render_grad_cases as RC
import render_grad_ref as R
# relative L2 per tensor against the float64 restatement.  Worst observed on this matrix (MI355X): NOT YET MEASURED; a float32
# torch evaluation of the same restatement stays <= 1.3e-6 (tests/test_render_grad_ref_cpu.py prints it)
from test_hip_render_grad import REL_TOL_FP64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import panic3d_amd
    panic3d_amd._lib.lib()
    return panic3d_amd


def _cu(t):
    return None if t is None else t.to(DEV).contiguous()


def _nchw(d):
    return d.permute(0, 1, 4, 2, 3).cpu()


def _forward_sigma(P, c, pts):
    """The library forward's densities, masks applied, at binary32 points [N,M,3] (the +-1000 sentinels are what is read)."""
    nhwc = P.ops.planes_to_nhwc(_cu(c["planes"]))
    opts = P.ops.make_opts(c["ro"], **c["kw"])
    sigma, _ = P.ops.triplane_decode(nhwc, _cu(pts), [_cu(t) for t in c["mlp"]], opts, density_only=True)
    return nhwc, opts, sigma[..., 0].cpu().numpy()


def _render_backward(P, c, nhwc, opts, **kw):
    return P.ops.render_backward(nhwc, _cu(c["rays_o"]), _cu(c["rays_d"]), _cu(c["depths"].reshape(-1, c["S"])), [_cu(t) for t in c["mlp"]],
                                 opts, [_cu(x) for x in c["cot"]], per_view_clamp=c["o"]["per_view"], **kw)


def _decode_backward(P, c, nhwc, opts, **kw):
    return P.ops.triplane_decode_backward(nhwc, _cu(c["coords"]), [_cu(t) for t in c["mlp"]], opts, _cu(c["g_sigma"]), _cu(c["g_rgb"]), **kw)


def _check(tag, dplanes, dmlp, ref):
    errs, stray, finite = R.gate_errors(_nchw(dplanes), [t.cpu() for t in dmlp], *ref)
    print(tag, {k: f"{v:.2e}" for k, v in errs.items()})
    assert finite, "gradient not finite"
    assert stray == 0, f"{stray} non-zero plane-gradient entries on texels no live sample taps"
    assert max(errs.values()) <= REL_TOL_FP64, errs


@pytest.mark.parametrize("case", RC.RENDER_CASES, ids=[c[0] for c in RC.RENDER_CASES])
def test_render_backward_edges(P, case):
    c = RC.build_render(case)
    nhwc, opts, sigma = _forward_sigma(P, c, RC.render_sigma_points(c))
    st = {}
    dplanes, dmlp = _render_backward(P, c, nhwc, opts, stats=st)
    assert dplanes.shape == nhwc.shape
    _check(f"render {c['name']}", dplanes, dmlp, RC.render_ref(c, sigma))
    rows = [x.abs().reshape(c["N"], c["R"], -1).sum(-1) != 0 for x in c["cot"] if x is not None]
    live_rays = int(torch.stack(rows).any(0).sum()) if rows else 0
    assert st["executed_samples"] <= live_rays * c["S"], st
    masked = RC.masks_from_sigma(sigma).reshape(c["N"], c["R"], c["S"])
    if c["name"] == "crop_cull":
        assert 0 < int(masked.all(-1).sum()) < c["R"], "the scene must hold fully masked rays (wsum == 0)"
    if c["name"] == "none":
        assert st["executed_samples"] == 0
        assert torch.count_nonzero(dplanes) == 0 and all(torch.count_nonzero(t) == 0 for t in dmlp)
    elif not c["o"]["binarize"]:
        assert st["executed_samples"] > 0


@pytest.mark.parametrize("case", RC.DECODE_CASES, ids=[c[0] for c in RC.DECODE_CASES])
def test_decode_backward_edges(P, case):
    c = RC.build_decode(case)
    nhwc, opts, sigma = _forward_sigma(P, c, c["coords"])
    st = {}
    dplanes, dmlp = _decode_backward(P, c, nhwc, opts, stats=st)
    _check(f"decode {c['name']}", dplanes, dmlp, RC.decode_ref(c, sigma))
    live = torch.zeros(c["N"], c["M"], dtype=torch.bool)
    for x in (c["g_sigma"], c["g_rgb"]):
        if x is not None:
            live |= x.abs().sum(-1) != 0
    assert st["executed_samples"] <= int(live.sum()), st
    if c["name"] == "none":
        assert st["executed_samples"] == 0
        assert torch.count_nonzero(dplanes) == 0 and all(torch.count_nonzero(t) == 0 for t in dmlp)


def _case(cases, name):
    return next(c for c in cases if c[0] == name)


def test_decoder_gradients_without_planes_and_twice(P):
    """want_planes=False: the same decoder-gradient bits; two calls at a ragged shape: the same decoder-gradient bits."""
    for build, run, case in ((RC.build_render, _render_backward, _case(RC.RENDER_CASES, "zeros")),
                             (RC.build_render, _render_backward, _case(RC.RENDER_CASES, "views_own")),
                             (RC.build_decode, _decode_backward, _case(RC.DECODE_CASES, "n2_m100"))):
        c = build(case)
        nhwc, opts, _ = _forward_sigma(P, c, RC.render_sigma_points(c) if "rays_o" in c else c["coords"])
        dp, a = run(P, c, nhwc, opts)
        none, b = run(P, c, nhwc, opts, want_planes=False)
        dp2, a2 = run(P, c, nhwc, opts)
        assert none is None and torch.count_nonzero(dp) > 0
        for x, y, z in zip(a, b, a2):
            assert torch.equal(x, y), "decoder gradients differ without the plane scatter"
            assert torch.equal(x, z), "decoder gradients must be bitwise reproducible"
        assert torch.allclose(dp, dp2, rtol=1e-5, atol=1e-6 * float(dp.abs().max()))


def test_output_contract_of_the_c_abi(P):
    """include/p3d_render_grad.h: d_planes_nhwc is accumulated into, the decoder gradients are overwritten, the workspace needs no
    initialisation — for both entry points, called through ctypes with valid small inputs."""
    L = P._lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def contract(call, wsb, plane_shape):
        def run(dplanes, fill, ws_byte):
            out = [torch.full(s, fill, device=DEV) for s in ((64, 32), (64,), (33, 64), (33,))]
            ws = torch.full((wsb,), ws_byte, dtype=torch.uint8, device=DEV)
            torch.cuda.synchronize()
            assert call(dplanes, out, ws) == 0
            torch.cuda.synchronize()
            return out, int(ws[:8].view(torch.int64).item())
        dplanes = torch.zeros(plane_shape, device=DEV)
        base, n0 = run(dplanes, 0.0, 0)
        once = dplanes.clone()
        assert n0 > 0 and torch.count_nonzero(once) > 0
        nan, n1 = run(dplanes, float("nan"), 0xFF)  # NaN-filled outputs, 0xFF-filled workspace, the un-zeroed plane gradient
        for a, b in zip(base, nan):
            assert torch.isfinite(b).all() and torch.equal(a, b), "decoder gradients must be overwritten, whatever the workspace held"
        assert n1 == n0, "executed_samples depends on the workspace's contents"
        assert torch.allclose(dplanes, 2 * once, rtol=1e-5, atol=1e-6 * float(once.abs().max())), "d_planes_nhwc must be accumulated into"

    c = RC.build_render(_case(RC.RENDER_CASES, "r63"))
    nhwc, opts, _ = _forward_sigma(P, c, RC.render_sigma_points(c))
    t = {k: _cu(c[k]) for k in ("rays_o", "rays_d")}
    depths, mlp, cot = _cu(c["depths"].reshape(-1, c["S"])), [_cu(x) for x in c["mlp"]], [_cu(x) for x in c["cot"]]
    wsb = L.p3d_render_backward_workspace_bytes(c["N"], c["R"], c["Sc"], c["Sf"])
    contract(lambda dpl, out, ws: L.p3d_render_backward_f32(p(nhwc), c["N"], c["H"], c["W"], p(t["rays_o"]), p(t["rays_d"]), c["R"], p(depths),
                                                            *(p(x) for x in mlp), C.byref(opts), *(p(x) for x in cot), p(dpl),
                                                            *(p(x) for x in out), p(ws), wsb, None), wsb, nhwc.shape)
    d = RC.build_decode(_case(RC.DECODE_CASES, "m65"))
    nhwc2, opts2, _ = _forward_sigma(P, d, d["coords"])
    coords, mlp2, gs, gr = _cu(d["coords"]), [_cu(x) for x in d["mlp"]], _cu(d["g_sigma"]), _cu(d["g_rgb"])
    wsb2 = L.p3d_triplane_decode_backward_workspace_bytes(d["N"], d["M"])
    contract(lambda dpl, out, ws: L.p3d_triplane_decode_backward_f32(p(nhwc2), d["N"], d["H"], d["W"], p(coords), d["M"], *(p(x) for x in mlp2),
                                                                     C.byref(opts2), p(gs), p(gr), p(dpl), *(p(x) for x in out), p(ws), wsb2,
                                                                     None), wsb2, nhwc2.shape)
