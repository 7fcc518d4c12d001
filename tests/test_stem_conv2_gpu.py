"""pmn_stem_conv2_f16s[_views] (FeatureNet conv0 + conv1 + conv2 in one launch, conv1's full-resolution map in LDS) against the two
launches it replaces, pmn_stem_f16s followed by pmn_conv2d_f16s (8 -> 16, 5x5, stride 2), on the same device: torch.equal, bit for
bit.  Shapes: smaller than one 16 x 16 half-resolution tile in one direction (every pixel a border and a padding case), partial
tiles on both edges, views x batch through the table of addresses, random weights, and a launch plan with the flag on and off."""
import re

import pytest
import torch

import goldenutil as GU
import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    import patchmatchnet_amd as P
    _, params, kw = GU.load_case("default")
    m = P.PatchmatchNet(**kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return m.cuda().eval()


def _two_launches(ops, img, p0, p1, p2):
    return ops.conv2d_f16s(ops.stem_f16s(img, *p0, *p1), *p2, 5, 2, relu=True)


def _packs(model):
    pk = model.feature._packed()
    return pk["conv0"], pk["conv1_f16s"], pk["conv2_f16s"]


@pytest.mark.parametrize("N,H,W", [(1, 24, 40), (1, 40, 24), (1, 72, 104), (2, 72, 104), (1, 71, 103), (1, 1, 1), (2, 33, 66)])
def test_tensor_form_is_stem_then_conv2_bit_for_bit(model, N, H, W):
    """24x40: fewer rows than a tile needs; 72x104 -> 36x52 half-res: partial tiles on both edges; 71x103 and 33x66: odd sizes and
    W % 4 != 0 (scalar staging); the base off by one float takes the scalar staging too and must give the same bits."""
    from patchmatchnet_amd import ops
    p0, p1, p2 = _packs(model)
    g = torch.Generator().manual_seed(H * 1000 + W)
    img = torch.rand(N, 3, H, W, generator=g).cuda()
    want = _two_launches(ops, img, p0, p1, p2)
    got = ops.stem_conv2_f16s(img, *p0, *p1, *p2)
    assert got.shape == want.shape == (N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 16)
    assert torch.equal(got, want)
    into = torch.full_like(want, -1.0)
    assert ops.stem_conv2_f16s(img, *p0, *p1, *p2, out=into) is into and torch.equal(into, want)
    buf = torch.empty(img.numel() + 1, device="cuda")
    shifted = buf[1:].view_as(img).copy_(img)
    assert torch.equal(ops.stem_conv2_f16s(shifted, *p0, *p1, *p2), want)


@pytest.mark.parametrize("V,B,H,W", [(3, 2, 72, 104), (2, 1, 37, 50)])
def test_table_form_reads_images_at_unrelated_addresses(model, V, B, H, W):
    """Views x batch through the device table (view / batch indexing, the tile order); 37x50: the scalar staging path."""
    from patchmatchnet_amd import ops
    p0, p1, p2 = _packs(model)
    g = torch.Generator().manual_seed(11)
    spacers, imgs = [], []
    for v in range(V):  # separately allocated, in an order unrelated to the view index
        spacers.append(torch.empty(1000 * (v + 1) + 4, device="cuda"))
        imgs.append(torch.rand(B, 3, H, W, generator=g).cuda())
    imgs = imgs[::-1]
    want = torch.cat([_two_launches(ops, im, p0, p1, p2) for im in imgs], 0)
    table = ops.SourceTable(torch.tensor([im.data_ptr() for im in imgs], dtype=torch.int64).cuda(), (V, B, 3, H, W))
    got = ops.stem_conv2_f16s_views(table, *p0, *p1, *p2)
    assert torch.equal(got, want)
    assert torch.equal(got, torch.cat([ops.stem_conv2_f16s(im, *p0, *p1, *p2) for im in imgs], 0))


def test_random_weights_128x160():
    """Random conv0 / conv1 / conv2 with BatchNorm statistics, inside the fp16-split domain (the packers raise F16DomainError
    otherwise), both entry points."""
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from patchmatchnet_amd import ops, params as PP
    g = torch.Generator().manual_seed(7)

    def bn(c):
        return (0.5 + torch.rand(c, generator=g), 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g),
                0.5 + torch.rand(c, generator=g))

    dev = lambda pair: tuple(torch.from_numpy(a).cuda() for a in pair)  # noqa: E731
    p0 = dev(PP.pack_conv(0.3 * torch.randn(8, 3, 3, 3, generator=g), bn=bn(8)))
    p1 = dev(PP.pack_stem_conv1_f16s(0.2 * torch.randn(8, 8, 3, 3, generator=g), bn=bn(8)))
    p2 = dev(PP.pack_conv_f16s(0.1 * torch.randn(16, 8, 5, 5, generator=g), bn=bn(16)))
    imgs = [(2.0 * torch.rand(1, 3, 128, 160, generator=g) - 0.5).cuda() for _ in range(2)]
    want = torch.cat([_two_launches(ops, im, p0, p1, p2) for im in imgs], 0)
    assert float(want.abs().max()) > 0.0
    assert torch.equal(torch.cat([ops.stem_conv2_f16s(im, *p0, *p1, *p2) for im in imgs], 0), want)
    table = ops.SourceTable(torch.tensor([im.data_ptr() for im in imgs], dtype=torch.int64).cuda(), (2, 1, 3, 128, 160))
    assert torch.equal(ops.stem_conv2_f16s_views(table, *p0, *p1, *p2), want)


def test_feature_net_with_and_without_the_flag(model):
    """FeatureNet.forward_hip: all three levels equal with fuse_stem_conv2 on and off (list of images: the per-image launches)."""
    g = torch.Generator().manual_seed(3)
    imgs = [torch.rand(1, 3, 72, 104, generator=g).cuda() for _ in range(3)]
    feat = model.feature
    assert feat.fuse_stem_conv2
    try:
        with torch.no_grad():
            on = feat.forward_hip(imgs)
            feat.fuse_stem_conv2 = False
            off = feat.forward_hip(imgs)
    finally:
        feat.fuse_stem_conv2 = True
    assert all(torch.equal(on[k], off[k]) for k in (1, 2, 3))


@pytest.mark.parametrize("in_place", [False, True])
def test_plan_replay_with_and_without_the_flag(model, in_place):
    """A PlannedForward at 64x80 recorded with fuse_stem_conv2 on and one recorded with it off: depth and confidence equal bit for bit
    under the same seed, on the recording call and on a replay; the plan with the flag on holds one launch fewer and no conv2."""
    from patchmatchnet_amd.graph import PlannedForward
    imgs, intr, extr, _ = synth.render_scene(3, 64, 80, seed=21, device="cuda")
    args = ([im.cuda().contiguous() for im in imgs], torch.as_tensor(intr).cuda(), torch.as_tensor(extr).cuda(),
            torch.tensor([425.0]).cuda(), torch.tensor([935.0]).cuda())
    feat = model.feature
    res, names = {}, {}
    try:
        for flag in (True, False):
            feat.fuse_stem_conv2 = flag
            slot = PlannedForward(model, inputs_in_place=in_place)
            outs = []
            with torch.no_grad():
                for step in range(2):
                    torch.manual_seed(900 + step)
                    o = slot(list(args[0]), args[1].clone(), *args[2:])
                    outs.append((o[0].clone(), o[1].clone()))
            torch.cuda.synchronize()
            assert slot.captures == 1 and slot.replays == 2
            res[flag], names[flag] = outs, next(iter(slot.cache.values()))[0].kernel_names()
    finally:
        feat.fuse_stem_conv2 = True
    for (d1, c1), (d0, c0) in zip(res[True], res[False]):
        assert torch.equal(d1, d0) and torch.equal(c1, c0)
    assert len(names[True]) == len(names[False]) - 1
    conv2 = re.compile(r"conv_f16s_kernel(?:ILi8ELi16ELi5ELi2E|<8, ?16, ?5, ?2,)")  # mangled or demangled
    assert any(conv2.search(n) for n in names[False]) and not any(conv2.search(n) for n in names[True])
    stems = 1 if in_place else 3  # one launch through the table of addresses, one per image otherwise
    assert sum("stem_f16s_kernel_conv2" in n for n in names[True]) == stems and not any("stem_f16s_kernel_conv2" in n for n in names[False])
