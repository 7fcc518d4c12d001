"""CPU checks of the PatchMatch kernel space (tests/kernel_space.py): every row selects the specialisation it declares (launch-plan
recording, no device), the rows jointly reach every instantiation the library compiles for the hot-path entry points, the float64
reference (tests/ref64.py) reproduces the reference's golden intermediates, and each row's tolerance is far below the error of a
plausible kernel mistake.  The device side is tests/test_kernel_space_gpu.py."""
import numpy as np
import pytest
import torch

import goldenutil as GU
import kernel_space as KS
import ref64 as R


def _lib():
    from patchmatchnet_amd import _lib
    return _lib


@pytest.mark.parametrize("row", KS.ROWS, ids=[r.id for r in KS.ROWS])
def test_row_records_its_kernel(row):
    rc, names = KS.record(row)
    if row.device_only and rc == -3:
        # > 48 KB of dynamic LDS: hipFuncSetAttribute needs a device, so without one nothing is recorded (the GPU test records it)
        assert names == [] and not torch.cuda.is_available()
        return
    assert rc == 0, rc
    assert names == [KS.mangle(row.kernel)], (row.kernel, names)


def test_rows_cover_every_reachable_instantiation():
    lib = _lib()
    inst = KS.library_instantiations(lib.LIB_PATH)  # raises when the library has no stubs
    dead = {KS.mangle(k) for k in KS.DEAD}
    assert dead <= set(inst), sorted(dead - set(inst))
    declared = {KS.mangle(r.kernel) for r in KS.ROWS}
    recorded = set()
    for r in KS.ROWS:
        rc, names = KS.record(r)
        recorded.update(names)
        if rc == -3 and r.device_only:
            recorded.add(KS.mangle(r.kernel))  # declared, checked by test_row_records_its_kernel and on the device
    others = {KS.mangle(k) for k in KS.OTHER_KERNELS}
    assert recorded == declared
    assert not dead & recorded, sorted(dead & recorded)
    missing = set(inst) - dead - recorded
    assert not missing, f"instantiations no row reaches: {sorted(missing)}"
    assert recorded - others == set(inst) - dead
    print(f"\nkernel space: {len(recorded - others)} reachable instantiations covered, {len(dead)} listed as dead, "
          f"of the library's {len(inst)}")


def test_mangling_and_symbol_reader():
    from oracle import oracle as O
    assert KS.mangle("gather_corr_kernel<64, 8, 0, 16, true>") == "_Z18gather_corr_kernelILi64ELi8ELi0ELi16ELb1EEv10GatherArgs"
    syms = KS.dynamic_symbols(_lib().LIB_PATH)
    assert "pmn_warp_correlate" in syms and "pmn_aggregate_regress" in syms
    with pytest.raises(AssertionError, match="no __device_stub__"):
        KS.library_instantiations(O.build())  # a shared object without kernels (the C oracle): fails, does not pass vacuously


# ---- the float64 reference against the reference's own intermediates (golden) and the fp32 oracle -------------------------------------

def _model(params, kw):
    import patchmatchnet_amd as P
    m = P.PatchmatchNet(**kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return m.eval()


@pytest.mark.parametrize("case", ["default", "variant", "counts"])
@pytest.mark.parametrize("stage", [3, 2, 1])
def test_ref64_reproduces_golden_intermediates(case, stage):
    """ref64 fed the golden inputs of every iteration reproduces the golden intermediates within the kernel tolerances (the golden
    values are the reference's fp32 tensors: what is left is fp32-vs-fp64 rounding), and its view-weight arg-max matches the oracle's
    wherever the top two responses are apart."""
    from oracle import oracle as O
    g, params, kw = GU.load_case(case)
    cfg = O.default_stage_configs(kw["patchmatch_interval_scale"], kw["propagation_range"], kw["patchmatch_iteration"],
                                  kw["patchmatch_num_sample"], kw["propagate_neighbors"], kw["evaluate_neighbors"])[stage]
    feats, proj, depth, vw = GU.stage_inputs(g, kw, stage)
    pm = getattr(_model(params, kw), f"patchmatch_{stage}")
    B, C, h, w = feats[0].shape
    rel = np.stack([np.matmul(proj[:, i], np.linalg.inv(proj[:, 0])) for i in range(1, proj.shape[1])], 1).astype(np.float32)
    eval_off = g[f"s{stage}_eval_offsets"]
    propa_off = g.get(f"s{stage}_propa_offsets")
    fw = R.feature_weight(feats[0], eval_off, pm._etable, pm.feature_weight_net, cfg.G)
    assert KS.error("feature_weight", g[f"s{stage}_feature_weight"], fw) < KS.TOL["feature_weight"][0]
    otr = []
    O.patchmatch_stage(cfg, params, feats[0], feats[1:], proj[:, 0], [proj[:, i] for i in range(1, proj.shape[1])], g["depth_min"],
                       g["depth_max"], depth, vw, noise=g["noise"] if stage == 3 else None, propa_offsets=propa_off,
                       eval_offsets=eval_off, trace=otr)
    for it in range(1, cfg.iterations + 1):
        key = f"s{stage}_it{it}_"
        is_inverse = stage == 1 and it == cfg.iterations
        propagate = cfg.propagate_neighbors > 0 and not is_inverse
        first = stage == 3 and it == 1
        d_in = depth if it == 1 else g[f"s{stage}_it{it - 1}_depth_out"]
        ds, xn = R.init_hypotheses(g["noise"] if first else None, None if first else d_in, 0, g["depth_min"], g["depth_max"],
                                   cfg.num_sample, cfg.interval_scale, propa_off if propagate else None,
                                   pm._ptable if propagate else None, h, w)
        assert KS.error("depth_sample", g[key + "depth_sample"], ds) < KS.TOL["depth_sample"][0]
        hyp = g[key + "depth_sample"]
        vw_in = None if first else (vw if it == 1 else g[f"s{stage}_it{it - 1}_view_weights"])
        ev = R.warp_correlate(feats[0], feats[1:], rel, hyp, vw_in, 0, pm.evaluation.similarity_net, pm.evaluation.pixel_wise_net,
                              cfg.G)
        assert KS.error("similarity", g[key + "similarity"], ev["similarity"]) < KS.TOL["similarity"][0]
        assert KS.error("view_weights", g[key + "view_weights"], ev["view_weights"]) < KS.TOL["view_weights"][0]
        if vw_in is None:
            r = np.sort(ev["responses"], axis=2)
            clear = (r[:, :, -1] - r[:, :, -2]) > 1e-5
            am = ev["responses"].argmax(axis=2)
            assert clear.mean() > 0.9
            np.testing.assert_array_equal(am[clear], otr[it - 1]["view_weight_argmax"][clear])
        cost = R.mlp(g[key + "similarity"], pm.evaluation.similarity_net, sigmoid=False)
        assert KS.error("cost", otr[it - 1]["cost"], cost) < KS.TOL["cost"][0]
        xn_ref = R.xnorm_of(hyp, g["depth_min"], g["depth_max"]).astype(np.float32)
        score, dep, _ = R.aggregate_regress(otr[it - 1]["cost"], hyp, xn_ref, g[f"s{stage}_feature_weight"], eval_off, pm._etable,
                                            cfg.interval_scale, is_inverse)
        assert KS.error("score", g[key + "score"], score) < KS.TOL["score"][0]
        assert KS.error("depth", g[key + "depth"], dep) < KS.TOL["depth"][0]


def test_ref64_confidence_and_normalisation_agree_with_the_oracle():
    from oracle import oracle as O
    for row in [r for r in KS.ROWS if r.op == "confidence"]:
        x = KS.inputs(row)
        ref = KS.reference(row, x)
        conf, idx = O.confidence(x["score"], (row.H, row.W))
        frac = ref["index_float"] - np.floor(ref["index_float"])
        clear = (np.minimum(frac, 1 - frac) > 1e-4) | (row.D == 1)  # where fp32 and fp64 truncate the regressed index alike
        assert clear.mean() > 0.9
        np.testing.assert_array_equal(idx[clear], ref["depth_index"][clear])
        assert KS.error("confidence", conf, ref["confidence"]) < KS.TOL["confidence"][0]
    row = [r for r in KS.ROWS if r.op == "normalize"][0]
    x = KS.inputs(row)
    want = (x["depth"] - x["depth_min"].reshape(-1, 1, 1, 1)) / (x["depth_max"] - x["depth_min"]).reshape(-1, 1, 1, 1)
    assert KS.error("normalized", want, KS.reference(row, x)["normalized"]) < KS.TOL["normalized"][0]


# ---- tolerances discriminate -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", KS.ROWS, ids=[r.id for r in KS.ROWS])
def test_tolerances_discriminate(row):
    """Every plausible mistake ref64 can express for the row moves one of the compared outputs by at least 10x its tolerance."""
    x = KS.inputs(row)
    mlps = KS.nets(row)
    ref = KS.reference(row, x, mlps)
    ms = KS.mistakes(row, x, ref, mlps)
    assert ms, row
    for name, (key, wrong) in ms.items():
        err = KS.error(key, wrong, ref[key])
        assert err > 10 * KS.TOL[key][0], f"{name}: error {err:.3e} on {key} is within 10x the tolerance {KS.TOL[key][0]:.1e}"
