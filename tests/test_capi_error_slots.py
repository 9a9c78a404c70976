"""The seven solver families of the library keep one last-error text each, per thread: a failure in one family's entry point
leaves what the other six families' *_last_error() return untouched, and a new thread starts with every text empty.  No GPU: every
call below fails on its arguments, before the library looks for a device."""
import ctypes as C
import threading

from nmpc_amd import _capi

ERR_INVALID_ARGUMENT = _capi.ERR_INVALID_ARGUMENT

# family -> the arguments of nmpc_hip_<family>_create with a NULL `out` (refused first, with "out ... is NULL")
CREATE_WITH_NULL_OUT = {
    "ddp": (b"cartpole", 10, 4, 0, None),
    "fmpc": (b"no_such_problem", 10, 4, 0, None),
    "cgmres": (b"no_such_problem", 10, 4, 0, None),
    "boxqp": (4, 4, 0, None),
    "gmres": (4, 4, 4, 0, None),
    "riccati": (4, 2, 10, 4, 0, None),
    "fmpc_step": (4, 2, 2, 10, 4, 0, None),
}
FAMILIES = tuple(CREATE_WITH_NULL_OUT)


def _library():
    L = C.CDLL(_capi.lib_path())  # function objects of its own: the mirrors set argtypes on theirs
    for f in FAMILIES:
        getattr(L, f"nmpc_hip_{f}_last_error").restype = C.c_char_p
    return L


def _texts(L):
    return {f: getattr(L, f"nmpc_hip_{f}_last_error")() for f in FAMILIES}


def _null_config(L, f):
    assert getattr(L, f"nmpc_hip_{f}_default_config")(None) == ERR_INVALID_ARGUMENT


def _null_out(L, f):
    assert getattr(L, f"nmpc_hip_{f}_create")(*CREATE_WITH_NULL_OUT[f]) == ERR_INVALID_ARGUMENT


def test_a_failure_in_one_family_leaves_the_other_families_texts():
    L = _library()
    for f in FAMILIES:
        _null_config(L, f)
    assert _texts(L) == {f: b"cfg is NULL" for f in FAMILIES}
    for failing in FAMILIES:
        before = _texts(L)
        _null_out(L, failing)
        after = _texts(L)
        assert b"out" in after[failing] and b"is NULL" in after[failing], (failing, after[failing])
        for f in FAMILIES:
            if f != failing:
                assert after[f] == before[f], f"a failure in {failing} changed the last error of {f}: {before[f]} -> {after[f]}"
        _null_config(L, failing)  # back to the text the other families still hold
    # the example of a shape check: a create that fails on its dimensions
    before = _texts(L)
    h = C.c_void_p()
    assert L.nmpc_hip_gmres_create(0, 4, 10, 0, C.byref(h)) == ERR_INVALID_ARGUMENT
    after = _texts(L)
    assert after["gmres"].startswith(b"[Gmres] n must be in")
    assert {f: t for f, t in after.items() if f != "gmres"} == {f: t for f, t in before.items() if f != "gmres"}


def test_a_new_thread_starts_with_empty_texts_and_keeps_its_own():
    L = _library()
    for f in FAMILIES:
        _null_config(L, f)
    mine = _texts(L)
    seen = {}

    def other_thread():
        try:
            seen["at_start"] = _texts(L)
            for f in FAMILIES:
                _null_out(L, f)
            seen["after_failures"] = _texts(L)
        except BaseException as e:  # re-raised below
            seen["error"] = e

    t = threading.Thread(target=other_thread)
    t.start()
    t.join()
    if "error" in seen:
        raise seen["error"]
    assert seen["at_start"] == {f: b"" for f in FAMILIES}
    assert all(b"is NULL" in seen["after_failures"][f] and b"out" in seen["after_failures"][f] for f in FAMILIES)
    assert _texts(L) == mine == {f: b"cfg is NULL" for f in FAMILIES}
