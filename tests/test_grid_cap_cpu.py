"""fgo_debug_grid_cap without a GPU: the largest grid that grid_for() (csrc/batch_call.hpp) hands out is 2^20 unless the hook lowers
it, values outside 1 .. 2^20 other than 0 change nothing, and 0 puts the default back.  tests/test_gpu_grid_stride.py relies on the
return value to know that its caps are in force."""
import graph_slam_amd as G

DEFAULT = 1 << 20


def test_the_default_is_2_to_the_20():
    assert G.lib.fgo_debug_grid_cap(0) == DEFAULT


def test_a_cap_holds_until_it_is_changed_and_zero_restores_the_default():
    cap = G.lib.fgo_debug_grid_cap
    try:
        assert cap(3) == 3
        assert cap(-1) == 3 and cap(DEFAULT + 1) == 3 and cap(-DEFAULT) == 3 and cap(2 ** 31 - 1) == 3      # not a cap: unchanged
        assert cap(1) == 1 and cap(DEFAULT) == DEFAULT and cap(DEFAULT - 1) == DEFAULT - 1                   # both ends of the range
        assert cap(0) == DEFAULT and cap(-1) == DEFAULT
    finally:
        assert cap(0) == DEFAULT
