"""CPU-side check of FeatureNet.fuse_stem_conv2 (no GPU): with the flag off forward_hip issues the launches it issued before the flag
existed, with it on the stem's and conv2's launches are one (pmn_stem_conv2_f16s[_views]) and everything after them is unchanged.
The ops are replaced by recorders that return tensors of the right shape."""
import torch

OPS = ["stem", "stem_f16s", "stem_f16s_views", "stem_conv2_f16s", "stem_conv2_f16s_views", "conv2d", "conv2d_f16s", "conv2d_f16s_pair",
       "pointwise_split_mfma", "fpn_level"]


def _launches(monkeypatch, flag, table=False):
    from patchmatchnet_amd import ops
    from patchmatchnet_amd.net import FeatureNet
    calls = []

    def half(n):
        return (n - 1) // 2 + 1

    def rec(name):
        def f(*a, **kw):
            x = a[0]
            if name in ("stem_f16s", "stem_conv2_f16s", "stem"):
                N, _, H, W = x.shape
                shape = (N, H, W, 8) if name != "stem_conv2_f16s" else (N, half(H), half(W), 16)
                out = kw.get("out")
                assert out is not None and tuple(out.shape) == shape, (name, shape)
                calls.append((name, shape))
                return out
            if name in ("stem_f16s_views", "stem_conv2_f16s_views"):
                V, B, _, H, W = x.shape
                shape = (V * B, H, W, 8) if name == "stem_f16s_views" else (V * B, half(H), half(W), 16)
            elif name == "conv2d_f16s":
                (N, H, W, _), s = x.shape, a[4]
                shape = (N, (H - 1) // s + 1, (W - 1) // s + 1, a[2].shape[0])
            elif name == "conv2d_f16s_pair":
                shape = tuple(x.shape)
            else:  # the head: two outputs nothing below looks into
                calls.append((name, None))
                return torch.empty(1), torch.empty(1)
            calls.append((name, shape))
            return torch.empty(shape)
        return f

    for n in OPS:
        monkeypatch.setattr(ops, n, rec(n))
    net = FeatureNet().eval()
    assert net.fuse_stem_conv2, "on by default"
    net.fuse_stem_conv2 = flag
    imgs = [torch.rand(2, 3, 24, 40) for _ in range(3)]
    if table:
        class Table:  # what forward_hip hands through to the _views op
            shape = (3, 2, 3, 24, 40)
        net.forward_hip(imgs, image_table=Table())
    else:
        net.forward_hip(imgs)
    assert net.f16_domain_error is None
    return calls


def test_flag_off_is_the_launch_list_of_before(monkeypatch):
    calls = _launches(monkeypatch, False)
    assert [c[0] for c in calls] == (["stem_f16s"] * 3 + ["conv2d_f16s", "conv2d_f16s_pair"] + ["conv2d_f16s"] * 6
                                     + ["pointwise_split_mfma", "fpn_level", "fpn_level"])
    assert calls[3][1] == (6, 12, 20, 16)
    calls = _launches(monkeypatch, False, table=True)
    assert [c[0] for c in calls][:3] == ["stem_f16s_views", "conv2d_f16s", "conv2d_f16s_pair"] and len(calls) == 12


def test_flag_on_has_one_launch_fewer(monkeypatch):
    off, on = _launches(monkeypatch, False, table=True), _launches(monkeypatch, True, table=True)
    assert len(on) == len(off) - 1
    assert on[0] == ("stem_conv2_f16s_views", (6, 12, 20, 16)) and on[1:] == off[2:]
    off, on = _launches(monkeypatch, False), _launches(monkeypatch, True)  # a list of images: the stem runs per image
    assert len(on) == len(off) - 1
    assert on[:3] == [("stem_conv2_f16s", (2, 12, 20, 16))] * 3 and on[3:] == off[4:]
