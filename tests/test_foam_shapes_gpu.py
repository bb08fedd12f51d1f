"""k_foam_update on the MI355X at the shapes the row walk treats differently: lane groups of 4 and 8 lanes (16^2, 32^2: several bands share a
wave and the launch ends in a partial wave), 1024^2 (a halo path), and launches whose texel count makes the host choose 8 and 32 rows per
band.  As in tests/test_foam_gpu.py the expectation is equality with the float32 restatement (tests/foam.py) on maps read back from the
same frames; _run_against_restatement is that module's, unchanged."""
import numpy as np
import pytest

import foam as FM
from test_foam_gpu import DT, _run_against_restatement, _time

pytestmark = pytest.mark.gpu
SHARE = (0.01, 0.30)                    # the generating-share window of tests/test_foam_gpu.py's single-tile cases


def _batch(n, tiles, mode="FULL7"):
    import watersurfacerendering_amd as W
    b = W.OceanBatch(n, tiles, 0)
    b.set_mode(getattr(W._abi, "OCEAN_MODE_" + mode))
    b.prepare(0x5EED0000 + n)
    return b


def _assert_band_rows(n, tiles, rows):
    """The shape reaches the band size it is here for on THIS part (the host's rule depends on the CU count).  A part with another CU count
    fails here, loudly, and the shapes get chosen again."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert FM.band_rows(n, tiles, cus) == rows, (n, tiles, cus, FM.band_rows(n, tiles, cus), rows)


# 16^2: on the Phillips sea of this size the default threshold (0.6) leaves at most 1.6 % of the texels generating and none at some
# steps; with 0.8 the restatement on oracle maps sits at 8 .. 14 % on every compared step.  32^2: 1.4 .. 3.3 % at the default.
@pytest.mark.parametrize("n,p_kw", [(16, dict(threshold=0.8)), (32, {})])
@pytest.mark.parametrize("mode", ["FULL7", "JACOBIAN"])
def test_small_tiles_with_narrow_lane_groups(n, p_kw, mode):
    """N / 4 = 4 or 8 lanes hold a row and wrap inside the group; 16 or 8 bands share a wave; 16 or 64 of the block's 256 threads work."""
    _assert_band_rows(n, 1, 4)
    b = _batch(n, 1, mode)
    _run_against_restatement(b, 1, 40, p_kw, SHARE, mode == "JACOBIAN", (n, mode))
    b.close()


def test_1024_single_tile():
    """256 column groups per row: four waves hold a row and take a halo float at each wave edge; rows = 4."""
    _assert_band_rows(1024, 1, 4)
    b = _batch(1024, 1)
    _run_against_restatement(b, 1, 10, {}, SHARE, False, (1024, "FULL7"))
    b.close()


def _run_selected_tiles(b, tiles, steps, tag):
    """_run_against_restatement for a launch of every tile of which only `tiles` are read back and restated (the others' maps and foam
    stay on the device): the same frames t_j = 0.1 j, one OCEAN_ALL_TILES update behind each, the share asserted and the foam compared
    for equality on every step.  Returns the restated foam of the selected tiles after the last step."""
    n = b.tile_size
    p = FM.params()
    dec = FM.decay(DT, p["lifetime"])
    want = {i: np.zeros((n, n), np.float32) for i in tiles}
    for j in range(steps):
        b.compute_waves(_time(j))
        b.update_foam(DT)
        for i in tiles:
            disp, nrm = b.read_maps(i, 1)
            jac = FM.jacobian(disp[0], nrm[0], -1.0, False)
            want[i] = FM.step(want[i], jac, p, dec)
            share = float((FM.generation(jac, p) > 0).mean())
            print(f"{tag} step {j + 1} tile {i}: generating share {share:.4f}, mean foam {float(want[i].mean()):.4f}")
            assert SHARE[0] <= share <= SHARE[1], (tag, j + 1, i, share)
            got = b.read_foam(i)
            assert np.array_equal(got, want[i]), (tag, j + 1, i, int((got != want[i]).sum()), float(np.abs(got - want[i]).max()))
    for i in tiles:
        assert 0.0 < float(want[i].mean()) < 0.6, (tag, i, float(want[i].mean()))
    return want


def test_eight_tiles_of_512_use_eight_rows_per_band():
    """8 x 512^2 = 2.1 M texels in one launch: rows = 8 on 256 compute units."""
    _assert_band_rows(512, 8, 8)
    b = _batch(512, 8)
    _run_selected_tiles(b, (0, 3, 7), 6, "8x512")
    b.close()


def test_eight_tiles_of_1024_use_32_rows_per_band_and_one_tile_uses_four():
    """8 x 1024^2 = 8.4 M texels in one launch: rows = 32 on 256 compute units.  One update of tile 5 alone on the same context is a launch
    with rows = 4: it equals one restated step from the state the 32-row launches left, and tile 4 keeps its state."""
    _assert_band_rows(1024, 8, 32)
    _assert_band_rows(1024, 1, 4)
    b = _batch(1024, 8)
    _run_selected_tiles(b, (0, 7), 3, "8x1024")
    before4, before5 = b.read_foam(4), b.read_foam(5)
    assert before4.mean() > 0 and before5.mean() > 0
    b.update_foam(DT, tile=5)
    disp, nrm = b.read_maps(5, 1)
    p = FM.params()
    jac = FM.jacobian(disp[0], nrm[0], -1.0, False)
    share = float((FM.generation(jac, p) > 0).mean())
    print(f"8x1024 tile 5 alone: generating share {share:.4f}")
    assert SHARE[0] <= share <= SHARE[1], share
    want5 = FM.step(before5, jac, p, FM.decay(DT, p["lifetime"]))
    got5 = b.read_foam(5)
    assert np.array_equal(got5, want5), (int((got5 != want5).sum()), float(np.abs(got5 - want5).max()))
    assert not np.array_equal(got5, before5)
    assert np.array_equal(b.read_foam(4), before4)
    b.close()
