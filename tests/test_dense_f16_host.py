"""The K-range arithmetic of connected_f16 (fp16 mode's dense layer, csrc/y2_dense_f16.hip) on the host: no device.

y2h_connected_f16_plan promises: the ranges are whole 32-steps except the last, which ends at `inputs`; they are disjoint,
ascending and cover [0, inputs); more than one range needs ranges * 16 * roundup(outputs, 16) fp32 partial sums, one range
needs none; a forced count is honoured up to the number of 32-steps.  The cost model's own choice is only held to those
promises, not to its constants."""
import numpy as np
import pytest

from sr_object_detection_amd import darknet

SHAPES = [(1, 512, 96), (16, 512, 96), (5, 96, 240), (3, 360, 50), (2, 54, 7), (17, 512, 96), (33, 512, 96),
          (1, 12544, 1470), (1, 25088, 4096), (16, 25088, 4096), (1, 50176, 512), (1, 12544, 1715), (1, 4096, 1000)]


def _check(rows, inputs, outputs, forced):
    n, ws, bounds = darknet.connected_f16_plan(rows, inputs, outputs, forced)
    steps = (inputs + 31) // 32
    assert 1 <= n <= steps and len(bounds) == n + 1
    assert bounds[0] == 0 and bounds[-1] == inputs
    assert (np.diff(bounds) > 0).all()                         # disjoint, ascending, none empty: they cover [0, inputs)
    assert (bounds[:-1] % 32 == 0).all()                       # every range but the last is whole 32-steps
    assert ws == (n * 16 * ((outputs + 15) // 16 * 16) * 4 if n > 1 else 0)
    return n


@pytest.mark.parametrize("rows,inputs,outputs", SHAPES)
def test_ranges_cover_the_inputs(rows, inputs, outputs):
    _check(rows, inputs, outputs, 0)


@pytest.mark.parametrize("rows,inputs,outputs", SHAPES)
@pytest.mark.parametrize("forced", [1, 2, 3, 7, 16, 1000000])
def test_forced_count_is_clamped_to_the_steps(rows, inputs, outputs, forced):
    assert _check(rows, inputs, outputs, forced) == min(forced, (inputs + 31) // 32)


def test_uneven_ranges_differ_by_one_step():
    _, _, bounds = darknet.connected_f16_plan(16, 512, 96, 7)           # 16 steps in 7 ranges
    assert set(np.diff(bounds) // 32) == {2, 3}
    _, _, bounds = darknet.connected_f16_plan(3, 360, 50, 5)            # 12 steps, the last one 8 wide
    assert bounds[-1] == 360 and bounds[-2] % 32 == 0


def test_large_layers_are_cut_for_the_whole_chip():
    """the weight-bound layers of the issue get more work items than the 92 .. 256 column tiles alone"""
    for inputs, outputs in ((12544, 1470), (25088, 4096), (50176, 512)):
        n = _check(1, inputs, outputs, 0)
        assert n > 1 and n * ((outputs + 15) // 16) >= 1024


def test_bad_arguments_are_refused():
    for args in ((0, 512, 96), (1, 0, 96), (1, 512, 0)):
        with pytest.raises(darknet.Y2Error):
            darknet.connected_f16_plan(*args)
