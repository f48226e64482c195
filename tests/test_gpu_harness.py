"""gpu_harness.py's conversions and identity front ends, on CPU tensors. CPU only."""
import numpy as np
import pytest
import torch

import gpu_harness as H

CPU = torch.device("cpu")


def test_to_device_keeps_dtype_and_is_contiguous():
    for dtype, tdtype in ((np.int32, torch.int32), (np.float64, torch.float64)):
        a = np.arange(12, dtype=dtype).reshape(3, 4)
        t = H.to_device(a, device=CPU)
        assert t.dtype == tdtype and t.is_contiguous() and t.shape == (3, 4) and np.array_equal(t.numpy(), a)
        v = H.to_device(a[:, 1:3], device=CPU)  # a strided view
        assert v.dtype == tdtype and v.is_contiguous() and np.array_equal(v.numpy(), a[:, 1:3])
    assert H.to_device(np.arange(3, dtype=np.int64), torch.int32, device=CPU).dtype == torch.int32
    assert H.to_device(np.arange(3), device=CPU).data_ptr() != 0


def test_to_device_gives_a_placeholder_for_an_empty_array():
    t = H.to_device(np.zeros(0, np.int32), device=CPU)
    assert t.dtype == torch.int32 and t.shape == (1,) and int(t[0]) == 0
    assert H.to_device(np.zeros((0, 6)), device=CPU).shape == (1,)


def test_to_host_drops_missing_outputs():
    out = dict(x=torch.tensor([1.0, np.nan], dtype=torch.float64), status=torch.tensor([0, 3], dtype=torch.int32),
               dual_res=None)
    h = H.to_host(out)
    assert set(h) == {"x", "status"} and h["status"].dtype == np.int32 and np.isnan(h["x"][1])


class _Ctx:
    def alloc_outputs(self, n):
        return dict(x=torch.empty((n, 3), dtype=torch.float64), status=torch.empty((n, 2), dtype=torch.int32))


def test_fresh_outputs_fill_guard_and_nb_out():
    out = H.fresh_outputs(_Ctx(), 4, nb_out=True)
    assert set(out) == {"x", "status", "nb_out"} and out["nb_out"].shape == (4, 16) and out["nb_out"].dtype == torch.int32
    assert bool(torch.isnan(out["x"]).all()) and bool((out["status"] == -7).all()) and bool((out["nb_out"] == -7).all())
    views, full = H.fresh_outputs(_Ctx(), 4, guard=8, fill=-77)
    assert views["x"].shape == (4, 3) and full["x"].shape == (12, 3) and bool((full["x"] == -77).all())
    views["status"].fill_(1)  # the views are the buffers' leading rows
    assert bool((full["status"][:4] == 1).all()) and bool((full["status"][4:] == -77).all())
    mixed = H.fresh_outputs(_Ctx(), 2, fill=(1e30, -7))
    assert bool((mixed["x"] == 1e30).all()) and bool((mixed["status"] == -7).all())


def test_identity_front_ends_take_tensors_dicts_and_rows():
    a = dict(x=torch.tensor([[0.0, np.nan], [1.0, 2.0]], dtype=torch.float64), status=torch.tensor([0, 3], dtype=torch.int32))
    b = {k: v.clone() for k, v in a.items()}
    H.same_bits(a, b)
    H.same_bits(a, {k: v.numpy().copy() for k, v in b.items()})  # tensors against their host copies
    H.same_values(a["x"], b["x"])
    b["x"][0, 0] = -0.0
    H.same_values(a, b, keys=("x", "status"))
    with pytest.raises(AssertionError, match="'x'"):
        H.same_bits(a, b)
    H.same_bits(a, b, rows=torch.tensor([1]))  # row 0 left out
    b["status"][1] = 4
    with pytest.raises(AssertionError, match="'status'"):
        H.same_values(a, b)
    H.same_values(a, b, rows=torch.tensor([0]))
