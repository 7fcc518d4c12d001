#!/usr/bin/env python
"""Stand-alone A/B: pmn_stem_conv2_f16s_views against pmn_stem_f16s_views + pmn_conv2d_f16s, six 1600x1200 views, back-to-back launches."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import goldenutil as GU
import patchmatchnet_amd as P
from patchmatchnet_amd import _lib
_, params, kw = GU.load_case("default")
model = P.PatchmatchNet(**kw)
model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
model = model.cuda().eval()
pk = model.feature._packed()
(w0, s0), (w1, s1), (w2, s2) = pk["conv0"], pk["conv1_f16s"], pk["conv2_f16s"]
L = _lib.lib()
V, H, W = 6, 1200, 1600
g = torch.Generator().manual_seed(1)
imgs = [torch.rand(1, 3, H, W, generator=g).cuda() for _ in range(V)]
tab = torch.tensor([im.data_ptr() for im in imgs], dtype=torch.int64).cuda()
mid = torch.empty(V, H, W, 8, device="cuda")
oa = torch.full((V, H // 2, W // 2, 16), -1.0, device="cuda")
ob = torch.full((V, H // 2, W // 2, 16), -2.0, device="cuda")
st = torch.cuda.current_stream().cuda_stream
p = lambda t: t.data_ptr()
def stem():
    assert L.pmn_stem_f16s_views(p(tab), V, p(w0), p(s0), p(w1), p(s1), p(mid), 1, H, W, st) == 0
def conv2():
    assert L.pmn_conv2d_f16s(p(mid), p(w2), p(s2), p(oa), V, H, W, 8, 16, 5, 2, 1, st) == 0
def two():
    stem(); conv2()
def fused():
    assert L.pmn_stem_conv2_f16s_views(p(tab), V, p(w0), p(s0), p(w1), p(s1), p(w2), p(s2), p(ob), 1, H, W, st) == 0
two(); fused(); torch.cuda.synchronize()
print("equal bits at 6x1200x1600:", bool(torch.equal(oa, ob)), flush=True)
res = {}
for rep in range(5):
    for name, run in (("stem", stem), ("conv2", conv2), ("two", two), ("fused", fused)):
        for _ in range(3):
            run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            run()
        e1.record()
        torch.cuda.synchronize()
        res.setdefault(name, []).append(1e3 * e0.elapsed_time(e1) / 20)
for k, v in res.items():
    print("us per six 1600x1200 views, 20 back-to-back launches, 5 rounds: %-6s %s" % (k, " ".join("%.1f" % x for x in v)), flush=True)
