"""Check of the tables a unit keeps in a scratch slot from call to call (csrc/common.h TableCache): whatever was called before, a call
gives the bits of the same call made first after qh_release_scratch - no table of an earlier key, no slot grown by an earlier call."""
from qampy_amd import _lib


def fresh(call):
    _lib.sync()
    _lib.call("qh_release_scratch")
    return call()


def assert_sequence_matches_fresh_calls(calls, seq):
    """calls: {name: callable returning an ndarray}; seq: the names in the order to call them.  Returns the fresh results by name."""
    want = {k: fresh(c) for k, c in calls.items()}
    _lib.sync()
    _lib.call("qh_release_scratch")
    for i, k in enumerate(seq):
        got = calls[k]()
        assert got.dtype == want[k].dtype and got.tobytes() == want[k].tobytes(), (i, k, seq)
    return want
