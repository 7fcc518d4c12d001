"""CPU-side checks of a launch plan's fork/join region (include/pmn_hip.h: pmn_plan_fork / _switch / _join / _entry_branch /
_launch_part): recording touches no device, so the markers, their error paths and the branch tags are checked here through ctypes
without a GPU, and so is the host-only overlap check of patchmatchnet_amd/ops.py.  Where a device is visible a replay launches for
real, so the one replay of recorded launches here runs in a child process that sees no device (tests/nodevice.py).  Replay:
tests/test_plan_branch_gpu.py; the recorder under sanitizers: tests/test_plan_host.py."""
import ctypes

import pytest

import nodevice


@pytest.fixture(scope="module")
def L():
    from patchmatchnet_amd import _lib
    try:
        return _lib.lib()
    except (_lib.PmnError, OSError) as e:
        pytest.skip(f"libpmn_hip.so does not load here: {e}")


def _plan(L):
    p = ctypes.c_void_p()
    assert L.pmn_plan_create(ctypes.byref(p)) == 0 and p.value
    return p


def test_markers_are_entries_and_carry_branch_tags(L):
    p = _plan(L)
    assert L.pmn_plan_begin(p) == 0
    assert L.pmn_plan_fork(p) == 0
    assert L.pmn_plan_switch(p, 1) == 0 and L.pmn_plan_switch(p, 0) == 0 and L.pmn_plan_switch(p, 1) == 0
    assert L.pmn_plan_join(p) == 0
    assert L.pmn_plan_end(p) == 0
    assert L.pmn_plan_count(p) == 2
    assert [L.pmn_plan_kernel_name(p, i) for i in range(2)] == [b"<fork>", b"<join>"]
    assert [L.pmn_plan_entry_branch(p, i) for i in range(2)] == [0, 0]
    assert L.pmn_plan_entry_branch(p, 2) == -1 and L.pmn_plan_entry_branch(p, -1) == -1 and L.pmn_plan_entry_branch(None, 0) == -1
    assert L.pmn_plan_kernel_name(p, 2) is None
    # nothing but markers: every part is empty, so replaying launches nothing (and needs no device)
    for part in range(4):
        assert L.pmn_plan_launch_part(p, part, None) == 0
    assert L.pmn_plan_launch(p, None) == 0
    assert L.pmn_plan_launch_part(p, 4, None) == -1 and L.pmn_plan_launch_part(p, -1, None) == -1
    assert L.pmn_plan_destroy(p) == 0


def test_marker_error_paths(L):
    p = _plan(L)
    # only while the calling thread records this plan
    assert L.pmn_plan_fork(p) == -1 and L.pmn_plan_switch(p, 1) == -1 and L.pmn_plan_join(p) == -1
    assert L.pmn_plan_fork(None) == -1 and L.pmn_plan_switch(None, 0) == -1 and L.pmn_plan_join(None) == -1
    assert L.pmn_plan_begin(p) == 0
    assert L.pmn_plan_join(p) == -1            # a join without a fork
    assert L.pmn_plan_switch(p, 1) == -1       # a switch outside a fork
    assert L.pmn_plan_fork(p) == 0
    assert L.pmn_plan_fork(p) == -1            # a nested fork
    assert L.pmn_plan_switch(p, 2) == -1 and L.pmn_plan_switch(p, -1) == -1
    assert L.pmn_plan_end(p) == -1             # pmn_plan_end with an open fork
    assert L.pmn_plan_launch(p, None) == -1    # ... leaves no usable plan
    assert L.pmn_plan_count(p) == 1 and L.pmn_plan_kernel_name(p, 0) == b"<fork>"
    assert L.pmn_plan_destroy(p) == 0

    q = _plan(L)  # (the failed end released this thread: it can record again)
    assert L.pmn_plan_begin(q) == 0 and L.pmn_plan_fork(q) == 0 and L.pmn_plan_join(q) == 0
    assert L.pmn_plan_fork(q) == -1            # one region per plan
    assert L.pmn_plan_switch(q, 1) == -1 and L.pmn_plan_join(q) == -1
    assert L.pmn_plan_end(q) == 0
    assert L.pmn_plan_fork(q) == -1            # sealed
    assert L.pmn_plan_destroy(q) == 0


def test_recorded_launches_take_the_current_branch(L):
    """Entry points called between the markers (fake device addresses: nothing is dereferenced while recording) are tagged with the
    branch that was current, and pmn_plan_count / pmn_plan_kernel_name / pmn_plan_entry_branch list the plan as recorded."""
    p = _plan(L)
    assert L.pmn_plan_begin(p) == 0
    assert L.pmn_nchw_to_nhwc(0x1000, 0x2000, 1, 4, 4, 4, None) == 0
    assert L.pmn_plan_fork(p) == 0
    assert L.pmn_normalize_depth(0x1000, 0x2000, 0x3000, 2, 100, 0x4000, None) == 0   # main until switched
    assert L.pmn_plan_switch(p, 1) == 0
    assert L.pmn_nchw_to_nhwc(0x5000, 0x6000, 1, 4, 4, 4, None) == 0
    assert L.pmn_nchw_to_nhwc(None, 0x6000, 1, 4, 4, 4, None) == -1                    # a refused call records nothing
    assert L.pmn_plan_switch(p, 0) == 0
    assert L.pmn_confidence(0x1000, 1, 8, 4, 4, 8, 8, 0x2000, None, None) == 0
    assert L.pmn_plan_join(p) == 0
    assert L.pmn_normalize_depth(0x1000, 0x2000, 0x3000, 2, 100, 0x4000, None) == 0
    assert L.pmn_plan_end(p) == 0
    n = L.pmn_plan_count(p)
    names = [L.pmn_plan_kernel_name(p, i).decode() for i in range(n)]
    tags = [L.pmn_plan_entry_branch(p, i) for i in range(n)]
    assert n == 7 and tags == [0, 0, 0, 1, 0, 0, 0], (names, tags)
    assert names[1] == "<fork>" and names[5] == "<join>"
    assert "nchw_to_nhwc_kernel" in names[0] and "normalize_depth_kernel" in names[2] and "nchw_to_nhwc_kernel" in names[3]
    assert "confidence" in names[4] and "normalize_depth_kernel" in names[6]
    assert L.pmn_plan_destroy(p) == 0
    # Replaying a part LAUNCHES its kernels on those addresses wherever a device is visible: what the side branch's launch answers
    # without one is asked of a child process that sees none (tests/nodevice.py), which records the fork region again.
    got = nodevice.run("""
        p = new_plan()
        assert L.pmn_plan_begin(p) == 0
        assert L.pmn_nchw_to_nhwc(0x1000, 0x2000, 1, 4, 4, 4, None) == 0
        assert L.pmn_plan_fork(p) == 0
        assert L.pmn_normalize_depth(0x1000, 0x2000, 0x3000, 2, 100, 0x4000, None) == 0
        assert L.pmn_plan_switch(p, 1) == 0
        assert L.pmn_nchw_to_nhwc(0x5000, 0x6000, 1, 4, 4, 4, None) == 0
        assert L.pmn_plan_switch(p, 0) == 0
        assert L.pmn_confidence(0x1000, 1, 8, 4, 4, 8, 8, 0x2000, None, None) == 0
        assert L.pmn_plan_join(p) == 0
        assert L.pmn_normalize_depth(0x1000, 0x2000, 0x3000, 2, 100, 0x4000, None) == 0
        assert L.pmn_plan_end(p) == 0
        tags = [L.pmn_plan_entry_branch(p, i) for i in range(L.pmn_plan_count(p))]
        rc = L.pmn_plan_launch_part(p, 1, None)
        L.pmn_plan_destroy(p)
        print("NODEVICE_JSON " + json.dumps({"tags": tags, "launch_part": rc}))
    """)
    assert got["tags"] == tags
    assert got["launch_part"] == -3  # no device there: the side branch's launch itself fails, loudly


def test_fork_marks_do_nothing_outside_a_plan_recording():
    from patchmatchnet_amd import ops
    assert ops._region() is None
    ops.plan_fork()
    ops.plan_switch(1)
    ops.plan_switch(0)
    ops.plan_join()
    assert ops._region() is None


def test_overlap_check_is_host_arithmetic():
    from patchmatchnet_amd import PmnError, ops
    a, b, c = (0x1000, 256), (0x1100, 256), (0x10ff, 2)  # c straddles the boundary of a and b
    ops.check_branch_overlap([a], [b], [a], [(0x2000, 64)])           # both read a, write apart: fine
    ops.check_branch_overlap([], [(0x1000, 0)], [a], [a])             # an empty range overlaps nothing
    with pytest.raises(PmnError, match="main branch writes"):
        ops.check_branch_overlap([], [c], [a], [])                    # main writes what side reads
    with pytest.raises(PmnError, match="main branch writes"):
        ops.check_branch_overlap([], [c], [], [b])                    # ... or writes
    with pytest.raises(PmnError, match="side branch writes"):
        ops.check_branch_overlap([b], [], [], [c])                    # the reverse
    with pytest.raises(PmnError, match="branch writes"):
        ops.check_branch_overlap([], [a], [], [a])
