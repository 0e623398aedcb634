"""The shapes the convolution-plan tests sweep (tests/test_conv_plan.py): every layer of the backbone and of the
super-resolution at batch 1, 2 and 4, plus small and ragged shapes.  A case is (N, I, O, H, W, up) with H, W the INPUT map."""

# (name, I, O, input resolution, up): the 3x3 layers of the flagship generator (bench.py: channel_base 32768, channel_max 512,
# 256^2 backbone; SuperresolutionHybrid8XDC with 256 hidden channels)
BACKBONE = [("b4.conv1", 512, 512, 4, 1)] + [
    (f"b{r}.conv{k}", i, o, r // 2 if k == 0 else r, 2 if k == 0 else 1)
    for r, i, o in ((8, 512, 512), (16, 512, 512), (32, 512, 512), (64, 512, 512), (128, 512, 256), (256, 256, 128))
    for k, i, o in ((0, i, o), (1, o, o))]
SUPERRES = [("sr.b0.conv0", 32, 256, 128, 2), ("sr.b0.conv1", 256, 256, 256, 1),
            ("sr.b1.conv0", 256, 128, 256, 2), ("sr.b1.conv1", 128, 128, 512, 1)]
TORGB = [(f"b{r}.torgb", min(512, 32768 // r), 96, r, 1) for r in (4, 8, 16, 32, 64, 128, 256)]


def model_cases():
    return [(n, i, o, r, r, up) for n in (1, 2, 4) for _, i, o, r, up in BACKBONE + SUPERRES + TORGB]


def ragged_cases():
    out = []
    for W in (4, 5, 8, 12, 16, 24, 31, 32, 33, 40, 64, 72, 128, 200, 512):
        for I, O in ((16, 32), (24, 40), (48, 96), (32, 64), (64, 48), (100, 60), (8, 3), (512, 512)):
            for up in (1, 2):
                if W >= 200 and I * O > 4096:
                    continue
                for N, H in ((1, W), (3, W // 2 + 1)):
                    out.append((N, I, O, H, W, up))
    return out


def all_cases():
    return model_cases() + ragged_cases()
