"""GPU tests of a launch plan with a side branch (include/pmn_hip.h pmn_plan_fork / _launch_part, graph.PlannedForward): the FPN's 1/4
and 1/2 levels and the offset heads and FeatureWeightNet of stages 2 and 1 replay on the plan's own stream beside stage 3, and every
depth and confidence map is still the eager forward's, bit for bit.  Inputs cycle from replay to replay: a missing join, or a buffer
the two branches share, then shows as a difference.  Shape: the smallest three-stage one of tests/test_plan_gpu.py (96x128), two
source views."""
import re

import pytest
import torch

import goldenutil as GU
import synth

pytestmark = pytest.mark.gpu

H, W, N_SRC, STEPS = 96, 128, 2, 12
NEIGHBOR = re.compile(r"gather_corr_kernel(?:ILi\d+ELi\d+ELi2E|<\d+, ?\d+, ?2,)")  # MODE_NEIGHBOR = 2: FeatureWeightNet


def _sample(seed):
    imgs, intr, extr, _ = synth.render_scene(N_SRC + 1, H, W, seed=seed, device="cuda")
    return dict(images=[im.cuda().contiguous() for im in imgs], intrinsics=torch.as_tensor(intr).cuda(),
                extrinsics=torch.as_tensor(extr).cuda(), depth_min=torch.tensor([425.0]).cuda(), depth_max=torch.tensor([935.0]).cuda())


def _call(f, s, **kw):
    out = f([im for im in s["images"]], s["intrinsics"].clone(), s["extrinsics"], s["depth_min"], s["depth_max"], **kw)
    return out[0], out[1]


@pytest.fixture(scope="module")
def case():
    """The model, three samples and the eager forward of step i (sample i % 3, draw seeded with 700 + i): computed once, read only."""
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    import patchmatchnet_amd as P
    _, params, kw = GU.load_case("default")
    model = P.PatchmatchNet(**kw)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    model = model.cuda().eval()
    samples = [_sample(30 + k) for k in range(3)]
    want = []
    with torch.no_grad():
        for i in range(STEPS):
            torch.manual_seed(700 + i)
            d, c = _call(model, samples[i % 3])
            want.append((d.clone(), c.clone()))
    torch.cuda.synchronize()
    return model, samples, want


def _replay_steps(slots, streams, samples):
    kept = []
    with torch.no_grad():
        for st in streams:
            st.wait_stream(torch.cuda.current_stream())
        for i in range(STEPS):
            torch.manual_seed(700 + i)
            with torch.cuda.stream(streams[i % len(streams)]):
                d, c = _call(slots[i % len(slots)], samples[i % 3])
                kept.append((d.clone(), c.clone()))
    torch.cuda.synchronize()
    return kept


def _differing(kept, want):
    return [i for i, (g, w) in enumerate(zip(kept, want)) if not (torch.equal(g[0], w[0]) and torch.equal(g[1], w[1]))]


def _listing(slot):
    handle = next(iter(slot.cache.values()))[0]
    names, tags = handle.kernel_names(), handle.entry_branches()
    assert handle.forked and len(names) == len(tags) == handle.count
    fork, join = names.index("<fork>"), names.index("<join>")
    assert names.count("<fork>") == names.count("<join>") == 1 and fork < join
    assert not any(tags[:fork + 1]) and not any(tags[join:]), "only entries between the markers are side-tagged"
    side = [n for n, t in zip(names[fork + 1:join], tags[fork + 1:join]) if t == 1]
    main = [n for n, t in zip(names[fork + 1:join], tags[fork + 1:join]) if t == 0]
    return names, side, main


@pytest.mark.parametrize("in_place", [False, True])
def test_forked_replays_on_a_side_stream_are_the_eager_forward(case, in_place):
    """(a) one slot on a non-default stream, 12 replays cycling three samples."""
    from patchmatchnet_amd.graph import PlannedForward
    model, samples, want = case
    slot = PlannedForward(model, inputs_in_place=in_place)
    kept = _replay_steps([slot], [torch.cuda.Stream()], samples)
    bad = _differing(kept, want)
    assert not bad, f"{len(bad)} of {STEPS} forked replays differ from the eager forward: {bad}"
    assert slot.captures == 1 and slot.replays == STEPS
    handle = next(iter(slot.cache.values()))[0]
    assert handle.forked and handle.side is not None, "the replay did not take the forked path"


def test_two_slots_in_flight(case):
    """(b) two slots on two streams, replays interleaved: four streams in all, each slot's side branch between its own events."""
    from patchmatchnet_amd.graph import PlannedForward
    model, samples, want = case
    slots = [PlannedForward(model, inputs_in_place=True) for _ in range(2)]
    kept = _replay_steps(slots, [torch.cuda.Stream() for _ in range(2)], samples)
    bad = _differing(kept, want)
    assert not bad, f"{len(bad)} of {STEPS} steps with two slots in flight differ from the eager forward: {bad}"
    sides = {next(iter(s.cache.values()))[0].side.cuda_stream for s in slots}
    assert len(sides) == 2, "every plan owns its side stream"


def test_the_same_plan_replays_on_one_stream_without_the_fork(case):
    """``fork=False``: pmn_plan_launch issues the forked plan's launches in recorded order on the caller's stream."""
    from patchmatchnet_amd.graph import PlannedForward
    model, samples, want = case
    slot = PlannedForward(model, fork=False)
    kept = _replay_steps([slot], [torch.cuda.Stream()], samples)
    assert not _differing(kept, want)
    assert next(iter(slot.cache.values()))[0].side is None


def test_branch_tags(case):
    """(c) side: the FPN's 1/4 and 1/2 levels, the offset heads and FeatureWeightNet of stages 2 and 1 -- nothing else; stage 3 is main."""
    from patchmatchnet_amd.graph import PlannedForward
    model, samples, _ = case
    slot = PlannedForward(model)
    with torch.no_grad():
        _call(slot, samples[0])
    torch.cuda.synchronize()
    names, side, main = _listing(slot)
    assert len(side) == 6, side
    assert sum("fpn_level_kernel" in n for n in side) == 2
    assert sum("conv_f16s_kernel" in n for n in side) == 2          # pmn_offset_heads_f16s: both heads of a stage in one launch
    assert sum(bool(NEIGHBOR.search(n)) for n in side) == 2
    # the FPN levels come first on the side branch (the heads read their output), 1/4 before 1/2
    assert "fpn_level_kernel" in side[0] and "fpn_level_kernel" in side[1]
    # stage 3 on the main branch: its heads, its FeatureWeightNet, and per iteration hypotheses, warp + correlate, aggregation
    assert not any("fpn_level_kernel" in n for n in main)
    assert sum("conv_f16s_kernel" in n for n in main) == 1 and sum(bool(NEIGHBOR.search(n)) for n in main) == 1
    assert sum("gather_corr_kernel" in n or "pixelwise_wave_kernel" in n for n in main) == 1 + 2
    assert len(main) == 2 + 3 * 2, main
    # before the fork: FeatureNet through the 1/8 level; after the join: stages 2 and 1 without heads, Refinement, confidence
    fork, join = names.index("<fork>"), names.index("<join>")
    assert any("stem_f16s_kernel" in n for n in names[:fork]) and not any("fpn_level_kernel" in n for n in names[:fork])
    assert not any(NEIGHBOR.search(n) for n in names[join:]) and any("refine_fused_kernel" in n for n in names[join:])
    assert "confidence" in names[-1]


def test_injected_features_fork_heads_only(case):
    """(d) ``features=``: FeatureNet is outside the plan, the side branch holds the heads and FeatureWeightNet of stages 2 and 1."""
    from patchmatchnet_amd.graph import PlannedForward
    model, samples, _ = case
    slot = PlannedForward(model)
    with torch.no_grad():
        for k in range(3):
            s = samples[k]
            f = model.feature.forward_hip(s["images"])
            feats = [{st: t[j:j + 1].permute(0, 3, 1, 2) for st, t in f.items()} for j in range(N_SRC + 1)]
            one = dict(s, images=[s["images"][0]] * (N_SRC + 1))
            torch.manual_seed(11 + k)
            want = _call(model, one, features=feats)
            torch.manual_seed(11 + k)
            got = _call(slot, one, features=feats)
            torch.cuda.synchronize()
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), k
    assert slot.captures == 1
    _, side, main = _listing(slot)
    assert len(side) == 4 and sum("conv_f16s_kernel" in n for n in side) == 2 and sum(bool(NEIGHBOR.search(n)) for n in side) == 2, side
    assert len(main) == 2 + 3 * 2, main


def test_overlap_check_fires_on_aliased_ranges():
    """(e) host only: two branches handed the same block.  Nothing is launched."""
    from patchmatchnet_amd import PmnError, ops
    x = torch.empty(1024, dtype=torch.float32, device="cuda")
    other = torch.empty(1024, dtype=torch.float32, device="cuda")
    whole, tail = ops._range(x), ops._range(x[512:])
    ops.check_branch_overlap([whole], [ops._range(other)], [whole], [])  # both only read x
    with pytest.raises(PmnError, match="must not share a buffer"):
        ops.check_branch_overlap([], [tail], [whole], [])                # main writes into what side reads
    with pytest.raises(PmnError, match="must not share a buffer"):
        ops.check_branch_overlap([whole], [], [], [tail])                # side writes into what main reads
    with pytest.raises(PmnError, match="must not share a buffer"):
        ops.check_branch_overlap([], [whole], [], [tail])                # both write
