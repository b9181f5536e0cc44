"""The prepack bracket's host-side contract (csrc/prepack.hip, include/mi355seg.h): one bracket per process at a time, refused with a clear
error and never with a crash; the paths taken here call no HIP function, so they run without a GPU."""
import ctypes
import threading

import pytest

import mi355seg

EINVAL = -1


@pytest.fixture()
def L():
    lib = mi355seg.lib()
    assert lib.query("mi355seg_prepack_active") == 0
    return lib


def _record_end(lib):
    plan, nbytes = ctypes.c_int(-1), ctypes.c_size_t(1)
    rc = lib.query("mi355seg_prepack_record_end", ctypes.byref(plan), ctypes.byref(nbytes), None, None, 0)
    return rc, plan.value, nbytes.value


def test_second_record_begin_is_refused_and_the_open_bracket_survives(L):
    assert L.query("mi355seg_prepack_record_begin") == 0
    try:
        assert L.query("mi355seg_prepack_record_begin") == EINVAL
        msg = L.query("mi355seg_last_error").decode()
        assert "mi355seg_prepack_record_begin" in msg and "a recording is open" in msg and "one bracket per process" in msg
        with pytest.raises(mi355seg.Mi355SegError, match="record_begin"):
            L.call("mi355seg_prepack_record_begin")
    finally:
        assert _record_end(L) == (0, 0, 0)           # the first bracket closes as if nothing had happened: nothing recorded, plan 0, 0 bytes
    assert _record_end(L)[0] == EINVAL               # (and is closed now)


def test_run_with_an_unknown_plan_is_einval(L):
    buf = ctypes.create_string_buffer(512)
    for plan in (0, -3, 1 << 20):
        assert L.query("mi355seg_prepack_run", plan, buf, 512, None) == EINVAL
        assert "unknown plan" in L.query("mi355seg_last_error").decode()
    assert L.query("mi355seg_prepack_active") == 0


def test_done_and_free_without_anything_to_do_return_ok(L):
    assert L.query("mi355seg_prepack_done", None) == 0
    assert L.query("mi355seg_prepack_free", 0) == 0
    assert L.query("mi355seg_prepack_free", 1 << 20) == 0
    assert L.query("mi355seg_prepack_jobs", 1 << 20) == 0


def test_two_threads_opening_a_bracket_one_wins_one_gets_the_error(L):
    """One attempt per thread, released together: exactly one record_begin succeeds, the other returns EINVAL with the message."""
    gate, out = threading.Barrier(2), [None, None]

    def attempt(i):
        gate.wait()
        rc = L.query("mi355seg_prepack_record_begin")
        out[i] = (rc, L.query("mi355seg_last_error").decode() if rc else "")      # (the message is the calling thread's)

    threads = [threading.Thread(target=attempt, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    try:
        assert sorted(rc for rc, _ in out) == [EINVAL, 0]
        assert "a recording is open" in [m for rc, m in out if rc][0]
    finally:
        assert _record_end(L) == (0, 0, 0)
