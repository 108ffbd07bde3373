"""The shared fp64 walk of the reader references (tests/blend_reference.py) on its own, not through the modules built on it: the record of the
hand-computable two-layer frame (tests/probe_reference.py hand_frame) at its centre pixel, against the numbers its docstring derives by hand.

Test infrastructure."""
import torch

import blend_reference as B
from helpers import O
from probe_reference import HAND_PX, HAND_PY, hand_frame


def centre_record(lv, cam):
    """The walk's record of the tile that holds pixel (HAND_PX, HAND_PY), and that pixel's row in it."""
    s0 = O.settings_from_camera(cam, torch.zeros(3), 3, 1.0, False)
    with torch.no_grad():
        aux = O.rasterize(lv["means"], None, lv["opac"], s0, colors_precomp=torch.full((2, 3), 0.5), scales=lv["scales"], rotations=lv["rot"],
                          return_aux=True)[3]
    for t in B.tiles(aux, s0, torch.float64):
        yy0, yy1, x0, x1 = t.window
        if yy0 <= HAND_PY < yy1 and x0 <= HAND_PX < x1:
            assert t.n == (yy1 - yy0) * (x1 - x0) and t.alpha.shape == (t.n, t.ids.shape[0]) and t.alpha.dtype == torch.float64
            return t, (HAND_PY - yy0) * (x1 - x0) + (HAND_PX - x0)
    raise AssertionError("no tile of the walk holds the centre pixel")


def check_centre(t, row):
    """Front entry first, whatever its index: both entries kept, weights 0.3 and 0.7 * 0.9 = 0.63, T after them 0.7 and 0.07, nothing terminates.
    1e-6: the scene's fp32 parameters are fed to an fp64 walk."""
    assert t.keep[row].tolist() == [True, True]
    assert t.dead[row].tolist() == [False, False] and t.term[row].tolist() == [False, False]
    w = (t.alpha_eff * t.Texcl)[row]
    for got, want in zip(w.tolist() + t.Tincl[row].tolist(), (0.3, 0.63, 0.7, 0.07)):
        assert abs(got - want) <= 1e-6, (got, want)
    assert float(t.Texcl[row, 0]) == 1.0 and float(t.Texcl[row, 1]) == float(t.Tincl[row, 0])
    # at the centre pixel both Gaussians sit on the pixel: G = 1, the uncapped opacity * G is the opacity
    assert float(t.dx[row].abs().max()) <= 1e-4 and float(t.dy[row].abs().max()) <= 1e-4 and float(t.power[row].abs().max()) <= 1e-6
    assert bool((t.a_raw[row] == t.alpha[row]).all()) and not bool(B.near_threshold(t)[row].any())


def test_the_walk_on_the_two_layer_frame():
    cam, lv = hand_frame("layers")
    t, row = centre_record(lv, cam)
    assert t.ids.tolist() == [1, 0]      # index 0 is the BACK Gaussian: the list position is not the index
    check_centre(t, row)
    # the same two Gaussians with their indices swapped: the same record under the other ids
    swapped = {k: v.flip(0) for k, v in lv.items()}
    t2, row2 = centre_record(swapped, cam)
    assert t2.ids.tolist() == [0, 1] and row2 == row
    check_centre(t2, row2)
    for k in ("power", "alpha", "Tincl", "Texcl"):
        assert torch.equal(getattr(t, k), getattr(t2, k)), k

