"""CPU: the preconditions of tests/test_gpu_craft_gather.py hold on the reference alone (the C oracle's run of scene T of
tests/event_scenes.py): at the epoch of the gather, 0.4 T_END, some but not all transitions and apsides have been found -- so the event
search's position and the used part of the event slabs matter -- and the craft's knot counts differ by more than a factor 2 -- so the
per-column row limits of the knot copy matter."""
import pytest

from test_gpu_craft_gather import FSAL_METHOD, METHOD, gather_preconditions


@pytest.mark.parametrize("method", [METHOD, FSAL_METHOD])
def test_scene_t_is_live_for_a_gather_at_two_fifths(method):
    gather_preconditions(method)
