"""The points argument of the six registration calls without a device: a torch tensor that is not on the device or an array
that is not (total, 3 or 4) is a ValueError of the manager's, raised before the library is called (a host pointer must
never reach it as a device pointer, with or without python -O)."""
import numpy as np
import pytest

from sgtd_amd import manager


class _NoLibrary:
    """stands where the library would: any call of it fails the test"""
    def __getattr__(self, name):
        raise AssertionError("the library was called: " + name)


@pytest.fixture
def h():
    m = manager.STDescManager.__new__(manager.STDescManager)
    m._L, m._h, m._nq = _NoLibrary(), None, 2
    return m


OFF = np.array([0, 5], np.int64)
QOFF = np.array([0, 2, 5], np.int64)
# every call that takes points, with arguments that are right but for the points
CALLS = {
    "register_clouds": lambda h, p: h.register_clouds(p, OFF, [0], [0]),
    "register_voxels": lambda h, p: h.register_voxels(p, OFF, [0, 1], [0], None, [0], [0]),
    "register_stored": lambda h, p: h.register_stored(p, OFF, [0], [3]),
    "register_stored_voxels": lambda h, p: h.register_stored_voxels(p, OFF, [0, 1], [3], None, [0], [0]),
    "register_loops_stored": lambda h, p: h.register_loops_stored(p, QOFF),
    "register_loops_local_stored": lambda h, p: h.register_loops_local_stored(p, QOFF),
}


def _host_tensor():
    import torch
    return torch.zeros((5, 3), dtype=torch.float32)


BAD_POINTS = {"host_tensor": _host_tensor, "n_by_2": lambda: np.zeros((5, 2), np.float32), "one_dim": lambda: np.zeros(15, np.float32)}


@pytest.mark.parametrize("bad", sorted(BAD_POINTS))
@pytest.mark.parametrize("call", sorted(CALLS))
def test_bad_points_are_a_value_error_before_the_library(h, call, bad):
    with pytest.raises(ValueError):      # (_NoLibrary's AssertionError: the library was reached)
        CALLS[call](h, BAD_POINTS[bad]())


def test_right_points_reach_the_library(h):
    """the arguments above are wrong in their points alone: with (5, 3) f32 every call gets as far as the library"""
    for call in sorted(CALLS):
        with pytest.raises(AssertionError, match="the library was called"):
            CALLS[call](h, np.zeros((5, 3), np.float32))
