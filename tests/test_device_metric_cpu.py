"""The metric in device memory, the parts that need no GPU: the buffer -> dict step of GbpEngine.eval / iterate_eval_each / ba_loop with
device=True (gbp_poplar_amd/_cabi.py: eval_buffer_views) on CPU tensors, and the TypeErrors raised before the library is called."""
import ctypes as C
import inspect

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gbp_poplar_amd import _cabi as cabi

# gbp_eval_out (include/gbp_mi355x.h) as a numpy record
EVAL_DT = np.dtype([("sum_norm", "<f8"), ("sum_half_sq", "<f8"), ("n_active", "<u8"), ("n_relin", "<u8"), ("n_robust", "<u8"),
                    ("n_nonfinite", "<u8"), ("n_nonpd", "<u8")])


def _records(n):
    rec = np.zeros(n, EVAL_DT)
    rec["sum_norm"] = 39.863837 * (1 + np.arange(n))
    rec["sum_half_sq"] = 4242224.19 / (1 + np.arange(n))
    rec["n_active"] = 3551 + np.arange(n)
    rec["n_relin"] = 7 * np.arange(n)
    rec["n_robust"] = 3478 - np.arange(n)
    rec["n_nonfinite"] = np.arange(n) % 2
    rec["n_nonpd"] = 2 ** 40 + np.arange(n)
    return rec


def test_the_record_is_seven_eight_byte_words():
    assert EVAL_DT.itemsize == 56 == C.sizeof(cabi.GbpEvalOut)
    assert cabi.EVAL_FIELDS == EVAL_DT.names == tuple(n for n, _ in cabi.GbpEvalOut._fields_)
    for name in EVAL_DT.names:
        assert EVAL_DT.fields[name][1] == getattr(cabi.GbpEvalOut, name).offset


def test_views_of_a_series_of_records():
    rec = _records(5)
    buf = torch.from_numpy(rec.view(np.int64).reshape(5, 7))
    v = cabi.eval_buffer_views(buf)
    assert tuple(v) == cabi.EVAL_FIELDS
    for k, name in enumerate(cabi.EVAL_FIELDS):
        t = v[name]
        assert t.shape == (5,) and t.dtype == (torch.float64 if name in ("sum_norm", "sum_half_sq") else torch.int64), name
        assert t.data_ptr() == buf.data_ptr() + 8 * k and t.stride() == (7,), name      # a view of column k: nothing copied
        assert np.array_equal(t.numpy().view(EVAL_DT[name]), rec[name]), name
    # ... views: what is written into the buffer later is what they show
    rec["sum_norm"][3] = -2.5
    rec["n_relin"][4] = 99
    assert v["sum_norm"][3].item() == -2.5 and v["n_relin"][4].item() == 99
    buf[0, 1] = torch.tensor(1.0, dtype=torch.float64).view(torch.int64)
    assert v["sum_half_sq"][0].item() == 1.0 and rec["sum_half_sq"][0] == 1.0


def test_views_of_one_record_have_length_one():
    rec = _records(3)[2:]
    buf = torch.from_numpy(rec.view(np.int64))
    assert buf.shape == (7,)
    v = cabi.eval_buffer_views(buf)
    for k, name in enumerate(cabi.EVAL_FIELDS):
        assert v[name].shape == (1,) and v[name].data_ptr() == buf.data_ptr() + 8 * k
        assert v[name].numpy().view(EVAL_DT[name])[0] == rec[name][0]
    assert cabi.eval_buffer_views(torch.zeros((0, 7), dtype=torch.int64))["n_active"].shape == (0,)


@pytest.mark.parametrize("bad", [torch.zeros(7, dtype=torch.int32), torch.zeros(7, dtype=torch.float64), torch.zeros((2, 8), dtype=torch.int64),
                                 torch.zeros((2, 3, 7), dtype=torch.int64), torch.zeros((), dtype=torch.int64)])
def test_views_refuse_what_is_not_a_record_buffer(bad):
    with pytest.raises(TypeError):
        cabi.eval_buffer_views(bad)


def test_a_buffer_that_cannot_take_device_records_is_a_type_error():
    dev = torch.device("cuda", 0)
    with pytest.raises(TypeError, match="CPU"):
        cabi.check_eval_buffer(torch.zeros(7, dtype=torch.int64), (7,), dev)
    with pytest.raises(TypeError, match="CPU"):
        cabi.check_eval_buffer(torch.zeros((4, 7), dtype=torch.int32), (4, 7), dev)
    with pytest.raises(TypeError, match="tensor"):
        cabi.check_eval_buffer(np.zeros(7, np.int64), (7,), dev)
    with pytest.raises(TypeError, match="tensor"):
        cabi.check_eval_buffer((cabi.GbpEvalOut * 2)(), (2, 7), dev)
    # the remaining checks do not depend on where the tensor lives: the meta device has no memory behind it
    meta = torch.device("meta")
    ok = torch.empty((4, 7), dtype=torch.int64, device=meta)
    assert cabi.check_eval_buffer(ok, (4, 7), meta) is ok
    with pytest.raises(TypeError, match="int64"):
        cabi.check_eval_buffer(torch.empty((4, 7), dtype=torch.int32, device=meta), (4, 7), meta)
    with pytest.raises(TypeError, match="shape"):
        cabi.check_eval_buffer(ok, (5, 7), meta)
    with pytest.raises(TypeError, match="shape"):
        cabi.check_eval_buffer(ok, (7,), meta)
    with pytest.raises(TypeError, match="contiguous"):
        cabi.check_eval_buffer(torch.empty((7, 4), dtype=torch.int64, device=meta).t(), (4, 7), meta)
    with pytest.raises(TypeError, match="lives on"):
        cabi.check_eval_buffer(ok, (4, 7), dev)


def test_the_three_calls_have_the_two_keywords():
    from gbp_poplar_amd.engine import GbpEngine
    for name in ("eval", "iterate_eval_each", "ba_loop"):
        p = inspect.signature(getattr(GbpEngine, name)).parameters
        assert p["device"].default is False and p["out"].default is None, name
