"""The frame stream on the census cost (mvsv_stream_set_census / DisparityStream.census):
96 x 40 frames, batch 2; each popped map equals compute_census of its pair, switching it
off gives compute again, the refusals, MODE_HH4, and the mean grid of a census frame."""
import numpy as np
import pytest

from oracle import twin
from tests import census_restate as cs

pytestmark = pytest.mark.gpu

INVALID_ARG = -1
W, H = 96, 40


@pytest.fixture(scope="module")
def frames(mvsv):
    return [mvsv.synth_pair(0xCE5500 + k, W, H, 0, 32) for k in range(5)]


def stream_matcher(mvsv, mode=0):
    return mvsv.StereoSGBM.create(0, 32, 5, 8, 32, 1, 31, 10, 20, 2, mode)


def run(st, pairs):
    got = []
    for L, R in pairs:
        if st.pending() == 4:
            got.append(st.pop())
        st.push(L, R)
    while st.pending():
        got.append(st.pop())
    return got


@pytest.mark.parametrize("mode", [0, 3], ids=["MODE_SGBM", "MODE_HH4"])
def test_stream_on_the_census_cost(gpu, mvsv, frames, mode):
    m = stream_matcher(mvsv, mode)
    p = {k: v for k, v in m.params().items() if k != "variant"}
    window = (9, 7)
    # the references: the one-shot entries, themselves held to the restatement for frame 0
    census_want = [m.compute_census(L, R, window=window) for L, R in frames]
    bt_want = [m.compute(L, R) for L, R in frames]
    assert np.array_equal(census_want[0], cs.compute(*frames[0], p, window))
    for a, b in zip(census_want, bt_want):
        assert not np.array_equal(a, b)  # the frames tell the two costs apart

    st = mvsv.DisparityStream(m, W, H, depth=4, batch=2, grid_roi=(0, 0, W, H))
    for k, (d, _) in enumerate(run(st, frames)):
        assert np.array_equal(d, bt_want[k]), f"BT frame {k}"
    st.census(window)
    for k, (d, means) in enumerate(run(st, frames)):  # five frames under batch 2: a partial group too
        assert np.array_equal(d, census_want[k]), f"census frame {k}"
        assert np.array_equal(means, twin.mean_disparity_grid(census_want[k])), f"census frame {k}: mean grid"
    # another window, then new parameters while census stays on
    st.census((5, 5))
    st.push(*frames[1])
    assert np.array_equal(st.pop()[0], m.compute_census(*frames[1], window=(5, 5)))
    m2 = stream_matcher(mvsv, mode)
    m2.setUniquenessRatio(0)
    st.set_params(m2)
    st.push(*frames[2])
    assert np.array_equal(st.pop()[0], m2.compute_census(*frames[2], window=(5, 5)))
    st.set_params(m)
    # a change while a frame is pending is refused, and the frame keeps its cost
    st.push(*frames[3])
    from mvstereovision3_amd import _lib
    assert _lib.lib().mvsv_stream_set_census(st._h, 0, 0) == INVALID_ARG
    assert _lib.lib().mvsv_stream_set_census(st._h, 9, 7) == INVALID_ARG
    with pytest.raises(mvsv.MvsvError, match="pending"):
        st.census(None)
    assert np.array_equal(st.pop()[0], m.compute_census(*frames[3], window=(5, 5)))
    # a refused window changes nothing
    with pytest.raises(mvsv.MvsvError, match="census window"):
        st.census((9, 9))
    st.push(*frames[4])
    assert np.array_equal(st.pop()[0], m.compute_census(*frames[4], window=(5, 5)))
    # StereoBM is refused while census is on
    with pytest.raises(mvsv.MvsvError, match="census"):
        st.set_params(mvsv.StereoBM.create(32, 9))
    assert st.matcher() == mvsv.MATCHER_SGBM
    # off: compute again
    st.census(None)
    for k, (d, means) in enumerate(run(st, frames[:3])):
        assert np.array_equal(d, bt_want[k]), f"BT frame {k} after census"
        assert np.array_equal(means, twin.mean_disparity_grid(bt_want[k]))
    st.set_params(mvsv.StereoBM.create(32, 9))  # allowed again
    with pytest.raises(mvsv.MvsvError, match="SGBM"):
        st.census(window)  # not with the BM matcher
    st.close()


def test_bm_and_colour_matching_streams_refuse_census(gpu, mvsv, frames):
    bm = mvsv.DisparityStream(mvsv.StereoBM.create(32, 9), W, H, depth=2)
    with pytest.raises(mvsv.MvsvError, match="SGBM"):
        bm.census((9, 7))
    bm.close()
    m = stream_matcher(mvsv)
    st = mvsv.DisparityStream(m, W, H, depth=2)
    st.enable_bgr((H, W), halve=False)
    st.bgr_match(True)
    with pytest.raises(mvsv.MvsvError, match="colour"):
        st.census((9, 7))
    st.bgr_match(False)
    st.census((9, 7))  # colour input prepared to grey is fine
    with pytest.raises(mvsv.MvsvError, match="census"):
        st.bgr_match(True)
    L, R = frames[0]
    st.push(L, R)
    assert np.array_equal(st.pop()[0], m.compute_census(L, R))
    # an int16 bound the window breaks is refused by name: blockSize 21, P2 5426, window (9, 7)
    big = mvsv.StereoSGBM.create(0, 32, 21, 10, 5426)
    with pytest.raises(mvsv.MvsvError, match="32767"):
        st.set_params(big)
    st.census(None)
    st.set_params(big)
    with pytest.raises(mvsv.MvsvError, match="32767"):
        st.census((9, 7))
    st.close()


def test_census_stream_with_optional_stages(gpu, mvsv, frames):
    """Display, sample points and the device map of a census frame follow the census map."""
    m = stream_matcher(mvsv)
    st = mvsv.DisparityStream(m, W, H, depth=2, grid_roi=(0, 0, W, H))
    st.enable_display()
    st.census((9, 7))
    L, R = frames[2]
    want = m.compute_census(L, R)
    st.push(gpu.from_numpy(L).cuda(), gpu.from_numpy(R).cuda())  # a device push takes the same path
    disp = st.front_display()
    d, means = st.pop()
    assert np.array_equal(d, want)
    shown = disp[0] if isinstance(disp, tuple) else disp
    ref = mvsv.normalize_minmax(gpu.from_numpy(want).cuda())
    ref = ref[0] if isinstance(ref, tuple) else ref
    assert np.array_equal(np.asarray(shown), ref.cpu().numpy())
    assert np.array_equal(means, twin.mean_disparity_grid(want))
    st.close()
