"""Every row of the PatchMatch kernel space (tests/kernel_space.py) on the device: the op through patchmatchnet_amd.ops, the plan the
device records for it (it selects the declared specialisation, including the rows whose dynamic LDS can only be raised with a device),
and every output against the float64 reference tests/ref64.py at the thresholds of tests/test_hip_parity.py's kernel tests
(kernel_space.TOL).  warp rows also run through pmn_warp_correlate_views, bit-identical to the stacked form.

MEASURED (first run on MI355X, maximum over the 96 rows of each error metric of kernel_space.TOL; per-row values are printed under
`-s`): depth_sample 1.5e-6 rel (init_hypotheses_kernel<16>, tolerance 2e-6), xnorm 1.6e-6 (2e-6), similarity 5.2e-6 (3e-5), view
weights 5.7e-7 (1e-5), cost 5.8e-6 scaled (5e-4), feature weight 9.4e-7 (2e-5), score 9.2e-6 (2e-4), depth 4.6e-6 rel (2e-5),
confidence 7.2e-8 (1e-6), normalised depth 5.6e-8 (1e-6).  No row needed a tolerance looser than test_kernels_against_golden's.
(cost's 5e-4 is set by ref64 against the golden intermediates, where the released weights amplify fp32 rounding of the MLP to
2.1e-4: tests/test_kernel_space.py.)"""
import numpy as np
import pytest
import torch

import goldenutil as GU
import kernel_space as KS
from oracle import oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ARGMAX_MARGIN = 1e-5  # arg-max over D compared where the float64 top two PixelwiseNet responses are further apart than this


def _gpu():
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    import patchmatchnet_amd as P
    P.lib()
    return P


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def n(x):
    return x.detach().cpu().numpy()


def _check(row, key, got, ref):
    err = KS.error(key, got, ref)
    print(f"MEASURED {row.id} {key} {err:.3e} (tolerance {KS.TOL[key][0]:.0e})")
    assert err < KS.TOL[key][0], f"{row.id}: {key} error {err:.3e} >= {KS.TOL[key][0]:.1e}"


@pytest.mark.parametrize("row", KS.ROWS, ids=[r.id for r in KS.ROWS])
def test_row_against_float64_reference(row):
    P = _gpu()
    rc, names = KS.record(row)  # with a device every row records, the > 48 KB LDS forms included
    assert rc == 0 and names == [KS.mangle(row.kernel)], (rc, names, row.kernel)
    x = KS.inputs(row)
    mlps = KS.nets(row)
    ref = KS.reference(row, x, mlps)
    dmin, dmax = t(x["depth_min"]), t(x["depth_max"])
    with torch.no_grad():
        if row.op == "init":
            ds, xn = P.ops.init_hypotheses(t(x["noise"]) if "noise" in x else None, t(x["depth"]) if "depth" in x else None,
                                           row.depth_shift, dmin, dmax, row.num_sample, float(x["interval_scale"]),
                                           t(x["propa_offsets"]) if row.propK else None, x.get("propa_table"), row.h, row.w)
            torch.cuda.synchronize()
            assert ds.shape[1] == row.D
            _check(row, "depth_sample", n(ds), ref["depth_sample"])
            _check(row, "xnorm", n(xn), ref["xnorm"])
        elif row.op == "feature_weight":
            fwn = mlps[2].to(DEV)
            fw = P.ops.feature_weight(t(x["ref_nhwc"]), t(x["eval_offsets"]), x["eval_table"], fwn.packed_device(), row.G)
            torch.cuda.synchronize()
            _check(row, "feature_weight", n(fw), ref["feature_weight"])
        elif row.op == "warp":
            sim_net, pix_net = mlps[0].to(DEV), mlps[1].to(DEV)
            src = t(x["src_nhwc"])
            args = (t(x["rel_proj"]), t(x["depth_sample"]), t(x["view_weights"]) if "view_weights" in x else None, row.vw_shift,
                    sim_net.packed_device(), pix_net.packed_device() if row.pixelwise else None, row.G)
            ref_nhwc = t(x["ref_nhwc"])
            cost, vw, am, sim = P.ops.warp_correlate(ref_nhwc, src, *args, want_similarity=True, want_argmax=row.pixelwise)
            table = P.ops.SourceTable(torch.tensor([src[v].data_ptr() for v in range(row.N)], dtype=torch.int64, device=DEV), src.shape)
            cost2, vw2, am2, sim2 = P.ops.warp_correlate(ref_nhwc, table, *args, want_similarity=True, want_argmax=row.pixelwise)
            torch.cuda.synchronize()
            _check(row, "similarity", n(sim), ref["similarity"])
            if row.pixelwise:
                _check(row, "view_weights", n(vw), ref["view_weights"])
            _check(row, "cost", n(cost), ref["cost"])
            for a, b in ((cost, cost2), (vw, vw2), (sim, sim2)):
                assert torch.equal(a, b), "pmn_warp_correlate_views differs from pmn_warp_correlate"
            if row.pixelwise:
                assert torch.equal(am, am2)
                r = np.sort(ref["responses"], axis=2)
                clear = (r[:, :, -1] - r[:, :, -2]) > ARGMAX_MARGIN if row.D > 1 else np.ones(r.shape[:2] + r.shape[3:], bool)
                # (far rows: hypotheses whose taps all miss the source give identical responses -- exact ties, left out)
                assert clear.mean() > (0.1 if row.far else 0.5)
                np.testing.assert_array_equal(n(am)[clear], ref["responses"].argmax(axis=2)[clear])
        elif row.op == "aggregate":
            score, dep = P.ops.aggregate_regress(t(x["cost"]), t(x["depth_sample"]), t(x["xnorm"]), t(x["feature_weight"]),
                                                 t(x["eval_offsets"]), x["eval_table"], float(x["interval_scale"]), row.is_inverse)
            torch.cuda.synchronize()
            _check(row, "score", n(score), ref["score"])
            _check(row, "depth", n(dep), ref["depth"])
        elif row.op == "confidence":
            conf, idx = P.ops.confidence(t(x["score"]), row.H, row.W, want_index=True)
            torch.cuda.synchronize()
            frac = ref["index_float"] - np.floor(ref["index_float"])
            clear = (np.minimum(frac, 1 - frac) > 1e-4) | (row.D == 1)  # fp32 and fp64 truncate the regressed index alike
            np.testing.assert_array_equal(n(idx)[clear], ref["depth_index"][clear])
            ys = np.minimum(np.floor(np.arange(row.H) * (row.h / row.H)).astype(np.int64), row.h - 1)
            xs = np.minimum(np.floor(np.arange(row.W) * (row.w / row.W)).astype(np.int64), row.w - 1)
            ok = clear[:, ys][:, :, xs]
            _check(row, "confidence", n(conf)[ok], ref["confidence"][ok])
        elif row.op == "normalize":
            out = P.ops.normalize_depth(t(x["depth"]), dmin, dmax)
            torch.cuda.synchronize()
            _check(row, "normalized", n(out), ref["normalized"])


def test_patchmatch_stage_at_a_configuration_no_release_uses():
    """The HIP cascade at num_sample [5, 20, 24], propagate [0, 8, 8], evaluate [17, 17, 9] (stage 3: 48 + 8 = 56 hypotheses ->
    init_hypotheses_kernel<64>, pixelwise_wave_kernel<2, false>; 17 evaluation neighbours at stages 1 and 2), one iteration per stage,
    seeded random offset heads, against the oracle on the same features and noise (as test_config0_one_iteration_per_stage_against_oracle)."""
    P = _gpu()
    _, params, kw = GU.load_case("default")
    kw = dict(kw, patchmatch_iteration=[1, 1, 1], patchmatch_num_sample=[5, 20, 24], propagate_neighbors=[0, 8, 8],
              evaluate_neighbors=[17, 17, 9])
    model = P.PatchmatchNet(**kw)
    sd = model.state_dict()
    gen = torch.Generator().manual_seed(5)
    new = {}
    for k, v in sd.items():
        if k in params and tuple(params[k].shape) == tuple(v.shape):
            new[k] = torch.from_numpy(params[k])
        else:  # offset heads of the neighbour counts the released weights do not have
            new[k] = 0.02 * torch.randn(v.shape, generator=gen)
    model.load_state_dict(new, strict=True)
    model = model.to(DEV).eval()
    params = {k: v.numpy() for k, v in new.items()}
    H, W = 64, 80
    from test_hip_parity import _rand_sample
    imgs, K, E, dmin, dmax = _rand_sample(3, H, W)
    noise = torch.rand(1, 48, H // 8, W // 8, generator=torch.Generator().manual_seed(22))
    with torch.no_grad():
        feats = model.extract_features(imgs)
        depth, conf, dpm = model([i.clone() for i in imgs], K.clone(), E, dmin, dmax, noise=noise.to(DEV), features=feats)
    feats_np = [{s: np.ascontiguousarray(n(f[s])) for s in (1, 2, 3)} for f in feats]
    cfgs = O.default_stage_configs(kw["patchmatch_interval_scale"], kw["propagation_range"], kw["patchmatch_iteration"],
                                   kw["patchmatch_num_sample"], kw["propagate_neighbors"], kw["evaluate_neighbors"])
    d1, _, out = O.cascade(params, feats_np, n(K), n(E), n(dmin), n(dmax), noise.numpy(), configs=cfgs)
    for stage in (3, 2, 1):
        assert len(dpm[stage]) == 1
        assert GU.rel_err(n(dpm[stage][0]), out[stage][0]) < 1e-3, stage
    assert GU.rel_err(n(dpm[1][0]), d1) < 1e-3
    assert bool(torch.isfinite(depth).all()) and bool(torch.isfinite(conf).all())
