"""GPU (-m gpu): training through the mapping network — FullyConnectedLayer's lrelu layers on the HIP bias_act forward / backward,
against the reference's fp32 autograd (tests/golden/mapping_grad.npz) and a float64 restatement; the memo layer around it; and G.f
with x['z'] under autograd: `backbone.mapping.*` receive what autograd.grad(ws, mapping parameters, ws_grad) gives."""
import pytest
import torch

import train_step_cases as TC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    panic3d_amd._lib.lib()
    return panic3d_amd


@pytest.mark.parametrize("L", TC.MAPPING_LAYERS)
def test_mapping_grad_vs_reference(P, L):
    TC.mapping_against_fixture(P, "cuda", L)


def test_mapping_grad_bits_and_memo(P):
    TC.mapping_bits_and_memo(P, "cuda")


def test_generator_f_with_z_trains_the_mapping_network(P):
    import p3d_shared_cases as MC
    import p3d_testing as T
    G = MC.memo_generator("cuda")
    T.fill_generator_params(G, 3)
    TC.fill_mapping(G, 4)
    G.set_view_replay(False)
    gen = torch.Generator().manual_seed(11)
    cond = {"image_ortho_front": torch.rand(1, 3, 32, 32, generator=gen).cuda(), "resnet_feats": torch.randn(1, 16, generator=gen).cuda()}
    z = torch.randn(1, G.backbone.z_dim, generator=gen).cuda()
    jit, u = T.make_random_draws(77, 1, 16 * 16, 12, 12)
    draws = (torch.from_numpy(jit).cuda(), torch.from_numpy(u).cuda())
    mk = lambda **o: dict(cond=cond, elevations=torch.zeros(1, device="cuda"), azimuths=torch.zeros(1, device="cuda"),
                          neural_rendering_resolution=16, noise_mode="const", triplane_crop=0.1, cull_clouds=0.5, **o)
    loss_of = lambda out: out["image_raw"].square().sum() + out["image_weights"].sum()
    mp = list(G.backbone.mapping.parameters())
    # the call under test: z in, a loss on the rendered outputs
    G._inject_draws = draws
    x = mk(z=z)
    out = G.f(x)
    assert x["ws"].grad_fn is not None
    loss_of(out).backward()
    got = [p.grad.clone() for p in mp]
    assert all(torch.isfinite(g).all() and torch.count_nonzero(g) > 0 for g in got)
    assert any(p.grad is not None for p in G.decoder.parameters())
    # the same call with ws as the leaf gives ws_grad; pulled back through the mapping alone
    G.zero_grad(set_to_none=True)
    ws_graph = G.mapping_zplus(z[:, None, :].expand(-1, G.backbone.num_ws, -1), torch.zeros(1, 25, device="cuda"), cond)
    ws_leaf = ws_graph.detach().clone().requires_grad_(True)
    assert torch.equal(ws_leaf, x["ws"].detach())
    G._inject_draws = draws
    loss_of(G.f(mk(ws=ws_leaf))).backward()
    want = torch.autograd.grad(ws_graph, mp, ws_leaf.grad)
    G._inject_draws = None
    for p, a, b in zip(G.backbone.mapping.named_parameters(), got, want):
        assert TC.rel_l2(a, b) <= 1e-6, p[0]
    # a seeds call under autograd never serves a memoised ws that lacks this call's graph
    with torch.no_grad():
        G._inject_draws = draws
        G.f(mk(seeds=[4]))
    G._inject_draws = draws
    xs = mk(seeds=[4])
    G.f(xs)
    G._inject_draws = None
    assert xs["ws"].grad_fn is not None
