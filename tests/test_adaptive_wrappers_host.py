"""CPU-only checks of the pure parts of the helper the solve_*_tsit5_adaptive* wrappers share (cloudy.jl_amd/_adaptive.py): the decoding
of the info planes with the RuntimeError of a batch that did not reach t_span, in the words of every wrapper, and the
normalisation of the save times."""
import numpy as np
import pytest

# the wrapper's name and what it integrates -> the message for statuses [0, 1, 0, 2]
MESSAGES = {
    ("solve_tsit5_adaptive", "parcel"):
        "solve_tsit5_adaptive: 2 of 4 parcels did not reach t_span; the first is parcel 1 (status 1: max_steps attempts)",
    ("solve_tsit5_adaptive_saveat", "parcel"):
        "solve_tsit5_adaptive_saveat: 2 of 4 parcels did not reach t_span; the first is parcel 1 (status 1: max_steps attempts)",
    ("solve_box_tsit5_adaptive", "parcel"):
        "solve_box_tsit5_adaptive: 2 of 4 parcels did not reach t_span; the first is parcel 1 (status 1: max_steps attempts)",
    ("solve_parcel_tsit5_adaptive", "parcel"):
        "solve_parcel_tsit5_adaptive: 2 of 4 parcels did not reach t_span; the first is parcel 1 (status 1: max_steps attempts)",
    ("solve_rainshaft_tsit5_adaptive", "column"):
        "solve_rainshaft_tsit5_adaptive: 2 of 4 columns did not reach t_span; the first is column 1 (status 1: max_steps attempts)",
    ("solve_rainshaft_tsit5_adaptive_saveat", "column"):
        "solve_rainshaft_tsit5_adaptive_saveat: 2 of 4 columns did not reach t_span; the first is column 1 (status 1: max_steps attempts)",
}


@pytest.fixture(scope="module")
def helper(cloudy):
    return cloudy._adaptive


@pytest.mark.parametrize("fn,what", sorted(MESSAGES))
def test_a_batch_that_did_not_reach_t_span_raises_in_the_wrappers_words(helper, fn, what):
    counts = np.array([[5, 7, 6, 3], [0, 2, 1, 4], [0, 1, 0, 2]], dtype=np.int32)
    with pytest.raises(RuntimeError) as e:
        helper.decode_info(fn, counts, what)
    assert str(e.value) == MESSAGES[(fn, what)]


def test_the_first_bad_status_is_named_with_its_words(helper):
    counts = np.array([[1, 1, 1], [0, 0, 0], [0, 0, 2]], dtype=np.int32)
    with pytest.raises(RuntimeError) as e:
        helper.decode_info("solve_tsit5_adaptive", counts)
    assert str(e.value) == ("solve_tsit5_adaptive: 1 of 3 parcels did not reach t_span; the first is parcel 2 (status 2: dt below 1e-14 "
                            "t_span or not finite)")
    assert helper.ADAPTIVE_STATUS == ("reached t_span", "max_steps attempts", "dt below 1e-14 t_span or not finite")


def test_a_batch_that_reached_t_span_gives_copies_of_the_rows(helper):
    counts = np.array([[5, 7, 6, 3], [0, 2, 1, 4], [0, 0, 0, 0]], dtype=np.int32)
    want = counts.copy()
    got = helper.decode_info("solve_tsit5_adaptive", counts)
    assert len(got) == 3
    for row, g in zip(want, got):
        assert isinstance(g, np.ndarray) and g.dtype == np.int32 and np.array_equal(g, row)
        assert not np.shares_memory(g, counts)
    counts[:] = -1
    for row, g in zip(want, got):
        assert np.array_equal(g, row)
    # an empty batch: nothing to raise about
    assert [g.size for g in helper.decode_info("solve_tsit5_adaptive", np.zeros((3, 0), np.int32))] == [0, 0, 0]


@pytest.mark.parametrize("name", ["saveat", "t_save", "times"])
def test_save_times(helper, name):
    one = helper.save_times(2.5, name)
    assert one.shape == (1,) and one.dtype == np.float64 and one[0] == 2.5
    several = helper.save_times([3, 1.5, 2], name)     # (the order is the caller's: the C entry point refuses a decreasing one)
    assert several.dtype == np.float64 and several.flags["C_CONTIGUOUS"] and several.tolist() == [3.0, 1.5, 2.0]
    strided = helper.save_times(np.arange(10, dtype=np.float32)[::3], name)
    assert strided.dtype == np.float64 and strided.flags["C_CONTIGUOUS"] and strided.tolist() == [0.0, 3.0, 6.0, 9.0]
    with pytest.raises(ValueError) as e:
        helper.save_times([[0.0, 1.0], [2.0, 3.0]], name)
    assert str(e.value) == f"{name} must be a sequence of times"
    for empty in ((), [], np.zeros(0)):
        ts = helper.save_times(empty, name)
        assert ts.shape == (0,) and ts.dtype == np.float64
        assert helper.save_args(ts, 64) == (0, None, None)   # n_save == 0: no pointers
    n_save, t_ptr, u_ptr = helper.save_args(several, 64)
    assert n_save == 3 and u_ptr == 64 and [t_ptr[i] for i in range(3)] == [3.0, 1.5, 2.0]
