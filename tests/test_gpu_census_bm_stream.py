"""The frame stream on the census StereoBM cost (mvsv_stream_set_bm_census /
DisparityStream.bm_census): 96 x 40 frames, batch 2; each popped map equals
compute_census of its pair, switching it off gives the SAD maps again, every refusal,
and the mean grid and display map of a census-BM frame."""
import numpy as np
import pytest

from oracle import twin
from tests import census_bm_restate as cb

pytestmark = pytest.mark.gpu

INVALID_ARG = -1
W, H = 96, 40


@pytest.fixture(scope="module")
def frames(mvsv):
    return [mvsv.synth_pair(0xCE5B00 + k, W, H, 0, 32) for k in range(5)]


def stream_matcher(mvsv, uniq=10):
    m = mvsv.StereoBM.create(32, 9)
    m.setUniquenessRatio(uniq)
    m._params.disp12_max_diff = 1
    m._params.speckle_window_size = 20
    m._params.speckle_range = 2
    return m


def run(st, pairs):
    got = []
    for L, R in pairs:
        if st.pending() == 4:
            got.append(st.pop())
        st.push(L, R)
    while st.pending():
        got.append(st.pop())
    return got


def test_stream_on_the_census_bm_cost(gpu, mvsv, frames):
    from mvstereovision3_amd import _lib
    m = stream_matcher(mvsv)
    p = {k: m.params()[k] for k in cb.PARAM_NAMES}
    window = (9, 7)
    # the references: the one-shot entries, themselves held to the restatement for frame 0
    census_want = [m.compute_census(L, R, window=window) for L, R in frames]
    sad_want = [m.compute(L, R) for L, R in frames]
    assert np.array_equal(census_want[0], cb.compute(*frames[0], p, window))
    for a, b in zip(census_want, sad_want):
        assert not np.array_equal(a, b)  # the frames tell the two costs apart

    st = mvsv.DisparityStream(m, W, H, depth=4, batch=2, grid_roi=(0, 0, W, H))
    assert st.matcher() == mvsv.MATCHER_BM
    for k, (d, _) in enumerate(run(st, frames)):
        assert np.array_equal(d, sad_want[k]), f"SAD frame {k}"
    st.bm_census(window)
    for k, (d, means) in enumerate(run(st, frames)):  # five frames under batch 2: a partial group too
        assert np.array_equal(d, census_want[k]), f"census frame {k}"
        assert np.array_equal(means, twin.mean_disparity_grid(census_want[k])), f"census frame {k}: mean grid"
    # another window, then new parameters while census stays on
    st.bm_census((5, 5))
    st.push(*frames[1])
    assert np.array_equal(st.pop()[0], m.compute_census(*frames[1], window=(5, 5)))
    m2 = stream_matcher(mvsv, uniq=0)
    st.set_params(m2)
    st.push(*frames[2])
    assert np.array_equal(st.pop()[0], m2.compute_census(*frames[2], window=(5, 5)))
    st.set_params(m)
    # a change while a frame is pending is refused, and the frame keeps its cost
    st.push(*frames[3])
    assert _lib.lib().mvsv_stream_set_bm_census(st._h, 0, 0) == INVALID_ARG
    assert _lib.lib().mvsv_stream_set_bm_census(st._h, 9, 7) == INVALID_ARG
    with pytest.raises(mvsv.MvsvError, match="pending"):
        st.bm_census(None)
    assert np.array_equal(st.pop()[0], m.compute_census(*frames[3], window=(5, 5)))
    # a refused window changes nothing
    with pytest.raises(mvsv.MvsvError, match="census window"):
        st.bm_census((9, 9))
    st.push(*frames[4])
    assert np.array_equal(st.pop()[0], m.compute_census(*frames[4], window=(5, 5)))
    # new parameters are held to the inherited rules while it is on
    with pytest.raises(mvsv.MvsvError, match="numDisparities"):
        st.set_params(mvsv.StereoBM.create(24, 9))
    # a switch to SGBM is refused while it is on, with the reason
    with pytest.raises(mvsv.MvsvError, match="census"):
        st.set_params(mvsv.StereoSGBM.create(0, 32, 5))
    assert st.matcher() == mvsv.MATCHER_BM
    # SGBM's own census call is not for this stream
    with pytest.raises(mvsv.MvsvError, match="SGBM"):
        st.census((9, 7))
    # off: the SAD maps again
    st.bm_census(None)
    for k, (d, means) in enumerate(run(st, frames[:3])):
        assert np.array_equal(d, sad_want[k]), f"SAD frame {k} after census"
        assert np.array_equal(means, twin.mean_disparity_grid(sad_want[k]))
    st.set_params(mvsv.StereoSGBM.create(0, 32, 5))  # allowed again
    with pytest.raises(mvsv.MvsvError, match="StereoBM"):
        st.bm_census(window)  # not with the SGBM matcher
    st.close()


def test_sgbm_streams_refuse_bm_census(gpu, mvsv, frames):
    st = mvsv.DisparityStream(mvsv.StereoSGBM.create(0, 32, 5, 8, 32), W, H, depth=2)
    with pytest.raises(mvsv.MvsvError, match="StereoBM"):
        st.bm_census((9, 7))
    with pytest.raises(mvsv.MvsvError, match="StereoBM"):
        st.bm_census(None)
    L, R = frames[0]
    st.push(L, R)
    assert st.pop()[0].shape == (H, W)
    st.close()


def test_census_bm_stream_with_optional_stages(gpu, mvsv, frames):
    """Display and the mean grid of a census-BM frame follow the census map."""
    m = stream_matcher(mvsv)
    st = mvsv.DisparityStream(m, W, H, depth=2, grid_roi=(0, 0, W, H))
    st.enable_display()
    st.bm_census((9, 7))
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
