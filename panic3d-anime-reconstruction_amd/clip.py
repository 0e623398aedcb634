"""CLIP's image tower on the HIP operators of include/p3d_clip.h: what `_scripts/eval/measure.py:34-43` uses for the
`clip` column of the evaluation table — `clip.load("ViT-B/32")`, the package's preprocessing of a PIL image, `encode_image` of both
images and the cosine of the two embeddings.

`CLIPVisual` is clip/model.py's VisionTransformer under OpenAI's `state_dict` names; `CLIPSimilarity` is measure.py's `clipsim` for a
batch of pairs.  Inference only.

Precision: the reference runs clip in float16 on CUDA, because `clip.load` converts the weights.  This implementation is binary32
throughout (float16 checkpoints are upcast when loaded); its similarities are therefore NOT the reference's bit for bit, and differ from
them by about the float16 network's own rounding error.

Neither the `clip` package nor its weights were available where this was written.  A freshly built model holds seeded random weights: it
is an image tower, not THE image tower, until `load_state_dict` is given the real arrays.  The architecture is pinned against
`transformers`' CLIPVisionModelWithProjection in float64 (tests/test_clip_cpu.py), the preprocessing against Pillow bit for bit.
Reading the real archive (`CLIPSimilarity(path)`) is best-effort and UNCHECKED.
"""
import torch

from . import memo, ops

EPS = 1e-5


class _LN(torch.nn.Module):
    def __init__(self, D):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(D), requires_grad=False)
        self.bias = torch.nn.Parameter(torch.zeros(D), requires_grad=False)


class _Linear(torch.nn.Module):
    def __init__(self, Ci, Co, std):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.randn(Co, Ci) * std, requires_grad=False)
        self.bias = torch.nn.Parameter(torch.zeros(Co), requires_grad=False)


class _Attention(torch.nn.Module):
    """torch.nn.MultiheadAttention's parameter names."""

    def __init__(self, D, std, proj_std):
        super().__init__()
        self.in_proj_weight = torch.nn.Parameter(torch.randn(3 * D, D) * std, requires_grad=False)
        self.in_proj_bias = torch.nn.Parameter(torch.zeros(3 * D), requires_grad=False)
        self.out_proj = _Linear(D, D, proj_std)


class _MLP(torch.nn.Module):
    def __init__(self, D, std, proj_std):
        super().__init__()
        self.c_fc = _Linear(D, 4 * D, std)
        self.c_proj = _Linear(4 * D, D, proj_std)


class ResidualAttentionBlock(torch.nn.Module):
    """x + attn(ln_1(x)), then x + mlp(ln_2(x)), mlp = c_proj(QuickGELU(c_fc(.)))  (containers of names only: never called)."""

    def __init__(self, D, layers):
        super().__init__()
        std, proj_std = D ** -0.5, (D ** -0.5) * ((2 * layers) ** -0.5)  # (clip/model.py initialize_parameters)
        self.ln_1, self.attn, self.ln_2, self.mlp = _LN(D), _Attention(D, std, proj_std), _LN(D), _MLP(D, (2 * D) ** -0.5, proj_std)


class _Transformer(torch.nn.Module):
    def __init__(self, D, layers):
        super().__init__()
        self.resblocks = torch.nn.Sequential(*[ResidualAttentionBlock(D, layers) for _ in range(layers)])


class _Conv1(torch.nn.Module):
    def __init__(self, D, patch):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.randn(D, 3, patch, patch) * (3 * patch * patch) ** -0.5, requires_grad=False)


class CLIPVisual(torch.nn.Module):
    """clip/model.py's VisionTransformer on the HIP path.

    encode_image(x): x [N,3,S,S] float32, already preprocessed -> the embedding [N,output_dim].  forward(img): img [N,C>=3,H,W] float32 in
    [0, 1] goes through clip's preprocessing first (8-bit quantisation, PIL's bicubic resize of the shorter side to image_size bit for
    bit, centre crop, normalisation).  fused=True walks the whole network in ONE call into the library; fused=False calls the operators
    step by step (the same kernels, the same bits).

    state_dict names are OpenAI's (152 tensors at the default configuration): conv1.weight, class_embedding, positional_embedding,
    ln_pre.*, transformer.resblocks.{i}.{ln_1.*, attn.in_proj_weight, attn.in_proj_bias, attn.out_proj.*, ln_2.*, mlp.c_fc.*, mlp.c_proj.*},
    ln_post.*, proj (used as x @ proj).  load_state_dict also takes them under a `visual.` prefix (a whole CLIP model's dict: the other
    entries are ignored) and in float16.  Every parameter has requires_grad=False.  The head dimension is 64: width = 64 * heads."""

    def __init__(self, width=768, layers=12, heads=12, image_size=224, patch_size=32, output_dim=512):
        super().__init__()
        self.width, self.layers, self.heads = int(width), int(layers), int(heads)
        self.image_size, self.patch_size, self.output_dim = int(image_size), int(patch_size), int(output_dim)
        if self.width != 64 * self.heads:
            raise ValueError(f"CLIPVisual: width {self.width} must be 64 * heads ({self.heads}): the attention kernel's head dimension is 64")
        if self.image_size % self.patch_size or self.layers < 1:
            raise ValueError("CLIPVisual: image_size must be a multiple of patch_size, and layers >= 1")
        self.tokens = 1 + (self.image_size // self.patch_size) ** 2
        if self.tokens > 64:
            raise ValueError(f"CLIPVisual: {self.tokens} tokens per image, the attention kernel takes at most 64")
        D, scale = self.width, self.width ** -0.5
        self.conv1 = _Conv1(D, self.patch_size)
        self.class_embedding = torch.nn.Parameter(scale * torch.randn(D), requires_grad=False)
        self.positional_embedding = torch.nn.Parameter(scale * torch.randn(self.tokens, D), requires_grad=False)
        self.ln_pre = _LN(D)
        self.transformer = _Transformer(D, self.layers)
        self.ln_post = _LN(D)
        self.proj = torch.nn.Parameter(scale * torch.randn(D, self.output_dim), requires_grad=False)
        self._operands, self._operands_key, self._programs, self._tab_key = None, None, {}, None

    # ---- parameters ------------------------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict=True, **kw):
        own = self.state_dict()
        sd = dict(state_dict)
        if any(k.startswith("visual.") for k in sd) and not any(k in own for k in sd):
            sd = {k[len("visual."):]: v for k, v in sd.items() if k.startswith("visual.")}
        sd = {k: (v.float() if isinstance(v, torch.Tensor) and v.dtype in (torch.float16, torch.bfloat16) else v) for k, v in sd.items()}
        return super().load_state_dict(sd, strict=strict, **kw)

    @staticmethod
    def convert_hf_state_dict(sd):
        """`transformers`' CLIPVisionModelWithProjection (or CLIPModel) names -> OpenAI's: q_proj / k_proj / v_proj are concatenated into
        in_proj_*, visual_projection.weight is transposed into proj.  Entries of the text tower are ignored."""
        out = {}
        v = "vision_model."
        out["conv1.weight"] = sd[v + "embeddings.patch_embedding.weight"]
        out["class_embedding"] = sd[v + "embeddings.class_embedding"]
        out["positional_embedding"] = sd[v + "embeddings.position_embedding.weight"]
        for ours, theirs in (("ln_pre", "pre_layrnorm"), ("ln_post", "post_layernorm")):  # ("pre_layrnorm": transformers' own spelling)
            for p in ("weight", "bias"):
                out[f"{ours}.{p}"] = sd[f"{v}{theirs}.{p}"]
        i = 0
        while f"{v}encoder.layers.{i}.layer_norm1.weight" in sd:
            a, b = f"{v}encoder.layers.{i}.", f"transformer.resblocks.{i}."
            for p in ("weight", "bias"):
                out[f"{b}attn.in_proj_{p}"] = torch.cat([sd[f"{a}self_attn.{n}_proj.{p}"] for n in ("q", "k", "v")])
                for ours, theirs in (("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"), ("attn.out_proj", "self_attn.out_proj"), ("mlp.c_fc", "mlp.fc1"),
                                     ("mlp.c_proj", "mlp.fc2")):
                    out[f"{b}{ours}.{p}"] = sd[f"{a}{theirs}.{p}"]
            i += 1
        out["proj"] = sd["visual_projection.weight"].t().contiguous()
        return out

    def blocks(self):
        return list(self.transformer.resblocks)

    def operands(self):
        """The operators' operands, derived from the parameters: ONE device blob that holds every weight in the order its kernel reads it
        ([K][Nout]: a Linear's weight transposed, conv1 as [3 patch^2][width]), every part on a 256-byte boundary, plus a tail that the
        walk's front end keeps its coefficient tables in; and {name: (offset, shape)}.  Cached under memo's convention — identity and
        `_version` of every parameter — so an in-place write (`copy_`, `load_state_dict`) re-derives them."""
        params = list(self.parameters())
        key = tuple((id(t), t._version, t.device) for t in params)
        if self._operands is None or self._operands_key != key or not memo.enabled():
            parts, index, at = [], {}, 0

            def put(name, t):
                nonlocal at
                t = t.detach().to(torch.float32).contiguous()
                index[name] = (at, tuple(t.shape))
                pad = -t.numel() % 64
                parts.append(t.reshape(-1))
                if pad:
                    parts.append(torch.zeros(pad, dtype=torch.float32, device=t.device))
                at += t.numel() + pad
            put("conv1", self.conv1.weight.reshape(self.width, -1).t())
            put("cls", self.class_embedding), put("pos", self.positional_embedding)
            put("ln_pre.w", self.ln_pre.weight), put("ln_pre.b", self.ln_pre.bias)
            for i, blk in enumerate(self.blocks()):
                for ln in ("ln_1", "ln_2"):
                    put(f"{i}.{ln}.w", getattr(blk, ln).weight), put(f"{i}.{ln}.b", getattr(blk, ln).bias)
                put(f"{i}.in_proj.w", blk.attn.in_proj_weight.t()), put(f"{i}.in_proj.b", blk.attn.in_proj_bias)
                for name, lin in (("out_proj", blk.attn.out_proj), ("c_fc", blk.mlp.c_fc), ("c_proj", blk.mlp.c_proj)):
                    put(f"{i}.{name}.w", lin.weight.t()), put(f"{i}.{name}.b", lin.bias)
            put("ln_post.w", self.ln_post.weight), put("ln_post.b", self.ln_post.bias)
            put("proj", self.proj)
            tail = 2 * self.image_size * (2 + TABLE_KSIZE)
            index["tables"] = (at, (tail,))
            parts.append(torch.zeros(tail, dtype=torch.float32, device=self.proj.device))
            self._operands, self._operands_key, self._programs, self._tab_key = (torch.cat(parts), index), key, {}, None
        return self._operands

    def operand(self, name):
        blob, index = self.operands()
        off, shape = index[name]
        n = 1
        for s in shape:
            n *= s
        return blob[off:off + n].view(*shape)

    # ---- the network as a list of step records ---------------------------------------------------------------------------------------
    def records(self, N, source=None, plan=0):
        """(records, buf_len, out) of a batch of N: the step records of ops.ClipProgram, the floats each arena buffer needs, and the
        (buffer, shape) of the embedding.  source = (C, H, W): the walk starts with the front end of such images (buffer 0); None: with
        the preprocessed batch (buffer 1).  Buffers: 0 the images, 1 the preprocessed batch, 2 the patch rows, 3 the residual stream,
        4 a normalised copy / the attention's output, 5 qkv, 6 the MLP's hidden rows, 7 the class tokens, 8 the embedding."""
        _, index = self.operands()
        off = lambda name: index[name][0]
        D, T, S, P, O = self.width, self.tokens, self.image_size, self.patch_size, self.output_dim
        M = N * T
        buf_len = [0, N * 3 * S * S, N * (T - 1) * D, M * D, M * D, M * 3 * D, M * 4 * D, N * D, N * O]
        recs = []
        if source is not None:
            Cc, H, W = source
            buf_len[0] = N * Cc * H * W
            pl = ops.clip_resize_plan(H, W, S)
            if pl["ksx"] > TABLE_KSIZE or pl["ksy"] > TABLE_KSIZE:
                raise ValueError(f"CLIPVisual: an image of {H} x {W} is reduced too much for the one-call walk; call it with fused=False")
            recs.append(dict(kind="prepare", name="prepare", src=0, dst=1, M=N, K=Cc, Nout=3, N=N, S=S, H=H, W=W, w=off("tables"),
                             b=off("tables") + S * (2 + pl["ksx"])))
        recs.append(dict(kind="gemm", name="conv1", src=1, dst=2, M=N * (T - 1), K=3 * P * P, Nout=D, N=N, S=S, patch=P, w=off("conv1"), plan=plan))
        recs.append(dict(kind="embed", name="ln_pre", src=2, dst=3, M=M, K=D, Nout=D, N=N, T=T, eps=EPS, w=off("ln_pre.w"), b=off("ln_pre.b"),
                         w2=off("cls"), b2=off("pos")))

        def ln(name, src, dst, rows=M, ld=D):
            recs.append(dict(kind="layernorm", name=name, src=src, dst=dst, M=rows, K=D, Nout=D, ld=ld, eps=EPS, w=off(name + ".w"), b=off(name + ".b")))

        def gemm(name, src, dst, K, Nout, res=None, gelu=False, bias=True, rows=M):
            recs.append(dict(kind="gemm", name=name, src=src, dst=dst, M=rows, K=K, Nout=Nout, res=res, gelu=gelu, w=off(name if not bias else name + ".w"),
                             b=off(name + ".b") if bias else None, plan=plan))
        for i in range(self.layers):
            ln(f"{i}.ln_1", 3, 4)
            gemm(f"{i}.in_proj", 4, 5, D, 3 * D)
            recs.append(dict(kind="attention", name=f"{i}.attn", src=5, dst=4, M=M, K=3 * D, Nout=D, N=N, T=T, heads=self.heads))
            gemm(f"{i}.out_proj", 4, 3, D, D, res=3)
            ln(f"{i}.ln_2", 3, 4)
            gemm(f"{i}.c_fc", 4, 6, D, 4 * D, gelu=True)
            gemm(f"{i}.c_proj", 6, 3, 4 * D, D, res=3)
        ln("ln_post", 3, 7, rows=N, ld=T * D)
        gemm("proj", 7, 8, D, O, bias=False, rows=N)
        return recs, buf_len, (8, (N, O))

    def program(self, N, source=None, plan=0):
        """The ops.ClipProgram of a batch size (and source size), cached with the operands."""
        blob, _ = self.operands()
        key = (int(N), None if source is None else tuple(int(v) for v in source), int(plan))
        if key not in self._programs or not memo.enabled():
            recs, buf_len, out = self.records(N, source, plan)
            prog = ops.ClipProgram(recs, buf_len, blob)
            prog.launches += sum(ops.clip_gemm_plan(r["M"], r["K"], r["Nout"], plan)["split"] > 1 for r in recs if r["kind"] == "gemm")
            self._programs[key] = (prog, out)
        return self._programs[key]

    def _check(self, x, what):
        if not isinstance(x, torch.Tensor) or x.ndim != 4 or x.shape[1] < 3:
            raise ValueError(f"CLIPVisual: expected {what}")
        if torch.is_grad_enabled() and x.requires_grad:
            raise NotImplementedError("CLIPVisual is inference only (measure.py calls it under torch.no_grad()): detach the image or call it "
                                      "under torch.no_grad()")
        if x.dtype != torch.float32:
            raise RuntimeError(f"x must be torch.float32, got {x.dtype}")
        return x.detach().contiguous()

    def _run(self, x, source, fused, plan):
        N = x.shape[0]
        if fused:
            prog, (buf, shape) = self.program(N, source, plan)
            if source is not None:  # the coefficient tables of this source size into the blob's tail (they stay until another size comes)
                tkey = (source[1], source[2])
                if self._tab_key != tkey:
                    blob, index = self.operands()
                    _, tabx, taby = ops.clip_prepare_tables(source[1], source[2], self.image_size, blob.device)
                    at = index["tables"][0]
                    for tab in (tabx, taby):
                        blob[at:at + tab.numel()].copy_(tab.reshape(-1).view(torch.float32))
                        at += tab.numel()
                    self._tab_key = tkey
            ops.clip_forward(prog, x, src=0 if source is not None else 1)
            return prog.buffer(buf, shape).clone()
        recs, _, (buf, _) = self.records(N, None, plan)
        op = self.operand
        bufs = {1: ops._clip_prepare_impl(x, self.image_size) if source is not None else x}
        for r in recs:
            src, name = bufs[r["src"]], r["name"]
            if r["kind"] == "gemm":
                res = bufs[r["res"]] if r.get("res") is not None else None
                w = op(name + ".w") if r.get("b") is not None else op(name)
                y = ops._clip_gemm_impl(src, w, op(name + ".b") if r.get("b") is not None else None, res, bool(r.get("gelu")), int(r.get("patch", 0)),
                                        int(r["plan"]), out=res)
            elif r["kind"] == "embed":
                y = ops._clip_embed_impl(src, op("cls"), op("pos"), N, op("ln_pre.w"), op("ln_pre.b"), EPS)
            elif r["kind"] == "layernorm":
                y = ops._clip_layernorm_impl(src, r["M"], r["K"], r["ld"], op(name + ".w"), op(name + ".b"), EPS)
            else:
                y = ops._clip_attention_impl(src, N, self.tokens, self.heads)
            bufs[r["dst"]] = y
        return bufs[buf]

    def encode_image(self, x, fused=True, plan=0):
        x = self._check(x, f"a preprocessed batch [N,3,{self.image_size},{self.image_size}]")
        if tuple(x.shape[1:]) != (3, self.image_size, self.image_size):
            raise ValueError(f"CLIPVisual: expected a preprocessed batch [N,3,{self.image_size},{self.image_size}], got {tuple(x.shape)}")
        with torch.no_grad():
            return self._run(x, None, fused, plan)

    def forward(self, img, fused=True, plan=0):
        img = self._check(img, "an image batch [N,C>=3,H,W] in [0, 1]")
        with torch.no_grad():
            source = tuple(int(v) for v in img.shape[1:])
            if fused and max(ops.clip_resize_plan(source[1], source[2], self.image_size)[k] for k in ("ksx", "ksy")) > TABLE_KSIZE:
                return self._run(ops._clip_prepare_impl(img, self.image_size), None, True, plan)  # (reduced more than 32 times: the front end on its own)
            return self._run(img, source, fused, plan)


TABLE_KSIZE = 129  # the widest coefficient row the blob's tail holds: a reduction by up to 32 (ksize = 2 ceil(2 scale) + 1)


def _load_state_dict(path):
    """A state dict from a file: torch.load (a pickled dict, or a model with .state_dict()), else the OpenAI TorchScript archive through
    torch.jit.load.  Best-effort and UNCHECKED: no such file was available."""
    try:
        obj = torch.load(path, map_location="cpu")
    except Exception:
        obj = torch.jit.load(path, map_location="cpu")
    if not isinstance(obj, dict):
        obj = obj.state_dict()
    return obj.get("state_dict", obj)


class CLIPSimilarity(torch.nn.Module):
    """measure.py:36-43's `clipsim` for a batch of pairs.  CLIPSimilarity(model_or_path)(a, b) -> [N]: a, b [N,C>=3,H,W] (or [C,H,W])
    float32 in [0, 1]; both go through clip's preprocessing and the image tower in one batch, then the cosine of embedding i of a and
    embedding i of b (a pair is a row of a against a row of b, not all against all).

    Inference only: an input that requires grad raises outside torch.no_grad().  Binary32, where the reference runs clip in float16 on
    CUDA (clip.load converts the weights): see the module's docstring.  model_or_path: a CLIPVisual, or the path of a checkpoint whose
    `visual.*` entries are loaded (unchecked)."""

    def __init__(self, model_or_path):
        super().__init__()
        if isinstance(model_or_path, CLIPVisual):
            self.model = model_or_path
        else:
            sd = _load_state_dict(model_or_path)
            pre = "visual." if any(k.startswith("visual.") for k in sd) else ""
            D, patch = sd[pre + "conv1.weight"].shape[0], sd[pre + "conv1.weight"].shape[-1]
            T = sd[pre + "positional_embedding"].shape[0]
            layers = len({k.split(".")[len(pre.split(".")) + 1] for k in sd if k.startswith(pre + "transformer.resblocks.")})
            self.model = CLIPVisual(D, layers, D // 64, round((T - 1) ** 0.5) * patch, patch, sd[pre + "proj"].shape[1])
            self.model.load_state_dict(sd if pre else {k: v for k, v in sd.items() if k in self.model.state_dict()})
        self.model.eval()

    def forward(self, a, b, fused=True):
        if not isinstance(a, torch.Tensor) or not isinstance(b, torch.Tensor):
            raise ValueError("CLIPSimilarity: two image tensors")
        a, b = (t[None] if t.ndim == 3 else t for t in (a, b))
        if a.ndim != 4 or a.shape[0] != b.shape[0]:
            raise ValueError(f"CLIPSimilarity: a {tuple(a.shape)} and b {tuple(b.shape)} must hold as many images each")
        if torch.is_grad_enabled() and (a.requires_grad or b.requires_grad):
            raise NotImplementedError("CLIPSimilarity is inference only (measure.py calls it under torch.no_grad())")
        with torch.no_grad():
            if a.shape[1:] == b.shape[1:]:
                e = self.model(torch.cat([a, b]), fused=fused)
                ea, eb = e[:a.shape[0]], e[a.shape[0]:]
            else:
                ea, eb = self.model(a, fused=fused), self.model(b, fused=fused)
            return ops._clip_cosine_impl(ea.contiguous(), eb.contiguous())
