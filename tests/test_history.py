"""What _binding.HistoryHandle and its helpers refuse before any device is touched."""
import importlib

import numpy as np
import pytest

binding = importlib.import_module("2022a-genome-dynamics_amd._binding")
Msd = importlib.import_module("2022a-genome-dynamics_amd.msd").Msd
Dcorr = importlib.import_module("2022a-genome-dynamics_amd.dcorr").Dcorr
Dmap = importlib.import_module("2022a-genome-dynamics_amd.dmap").Dmap


@pytest.mark.parametrize("cls", [binding.HistoryHandle, Msd, Dcorr, Dmap])
def test_set_history_refuses_frames_that_are_not_triples(cls):
    assert cls.set_history is binding.HistoryHandle.set_history
    h = cls.__new__(cls)      # no handle behind it: the shape is refused before the library is called
    for shape in [(4, 5, 2), (5, 3), (2, 4, 5, 3)]:
        with pytest.raises(ValueError) as e:
            h.set_history(np.zeros(shape, np.float32))
        assert str(e.value) == f"history must be (F, N, 3), got {shape}"


def test_u32_refuses_what_is_no_uint32():
    for bad in [[-1, 2], [0.0, 1.0], [1, 2.5], [0, 1 << 32], np.array([3, -7], np.int64), [True, False]]:
        with pytest.raises(ValueError) as e:
            binding._u32(bad, "lags")
        assert str(e.value) == "lags must be integers in [0, 2^32)"
    got = binding._u32([[0, 7], [7, (1 << 32) - 1]], "chain ranges")
    assert got.dtype == np.uint32 and got.flags.c_contiguous and got.tolist() == [[0, 7], [7, 4294967295]]
    assert binding._u32([], "lags").shape == (0,)


def test_ratio_broadcasts_the_count_and_leaves_nan_where_it_is_zero():
    total = np.arange(12, dtype=np.float64).reshape(2, 2, 3)
    count = np.array([[2, 0, 4], [0, 1, 8]], np.uint64)
    got = binding._ratio(total, count[None])
    want = np.array([[[0, np.nan, 0.5], [np.nan, 4, 0.625]], [[3, np.nan, 2], [np.nan, 10, 1.375]]])
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(binding._ratio(total[0], count), want[0])
