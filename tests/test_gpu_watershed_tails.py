"""Both tail kernels of the watershed on the serpentine lake (frames and reference: test_watershed_tails_cpu.py).

The lake's component holds two marker ids, so its frames go on to the second level, where K2 has to travel from q1 along the
whole corridor, one round per tile crossing: dozens of rounds against WS_K2_GRID_ROUNDS = 4, so the keys come out of
ws_k2_relax_tail_kernel -- as the levels before them come out of ws_relax_tail_kernel (12 grid rounds).  With the lake in
frames 0 and 2 of three the second level's frame list is {0, 2}.  192 x 192 takes the 16-byte tile loads and stores of the
relaxation, 192 x 190 (W % 4 != 0) the scalar ones and ws_uf_label_kernel.

Not covered: the overflow branch of the tail list (more than 1 024 marked tiles in one frame needs a frame of at least
2 048 x 2 048)."""
import numpy as np
import pytest

from test_watershed_tails_cpu import LAKE_FRAMES, SHAPES, batch

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _run(shape, mode):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")
    from particle_col_image_segmentation_amd import ops
    img, markers, mask, ref = batch(shape)
    out, flags = ops.watershed(torch.from_numpy(img.copy()).cuda(), torch.from_numpy(markers.copy()).cuda(),
                               torch.from_numpy(mask.astype(np.uint8)).cuda(), mode=mode)
    torch.cuda.synchronize()
    return out.cpu().numpy(), flags.cpu().numpy(), ref


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_second_level_resolves_the_lake_in_its_tail_kernel(shape):
    """Mode 2 (no exact flood): the lake frames come back unflagged and equal to the reference, so the second level
    resolved them."""
    out, flags, ref = _run(shape, 2)
    print("tie_flags:", flags.tolist())
    for b in LAKE_FRAMES:
        print("frame %d: %d pixels differ from the reference" % (b, int((out[b] != ref[b]).sum())))
    for b in LAKE_FRAMES:
        assert flags[b] == 0, flags.tolist()
        np.testing.assert_array_equal(out[b], ref[b], err_msg="frame %d" % b)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_all_frames_equal_the_reference_in_mode_0(shape):
    out, _, ref = _run(shape, 0)
    for b in range(3):
        np.testing.assert_array_equal(out[b], ref[b], err_msg="frame %d" % b)
