"""``espm_amd._image.on_device``, the one place where an image reaches the GPU, on its own (every analysis tests it through its
results only).

Shape: X of 5 x 37 - odd in both directions, more than one row, small enough that every case is a few milliseconds; with the chunk
of the host upload patched to 80 entries it goes up in steps of 2, 2 and 1 rows, a ragged last step.  Values: the extremes of every
integer dtype that the target holds exactly (64-bit integers up to 2^53), halves for the floating-point dtypes - so "exactly equal"
is a statement about the conversion and not about friendly values."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPE = (5, 37)
# the as-measured rule, written out: dtype of X -> dtype on the device
TABLE = {"bool": "uint8", "uint8": "uint8", "int8": "float32", "uint16": "uint16", "int16": "float32", "int32": "float64",
         "uint32": "float64", "int64": "float64", "float16": "float32", "float32": "float32", "float64": "float64"}
READ_AS_THEY_ARE = ["uint8", "uint16", "float32", "float64"]


@pytest.fixture(scope="module")
def image():
    from espm_amd import _image
    return _image


def _codes():
    from espm_amd import _lib
    return {"uint8": _lib.DIAG_X_U8, "uint16": _lib.DIAG_X_U16, "float32": _lib.DIAG_X_F32, "float64": _lib.DIAG_X_F64}


def _host(dtype):
    rng = np.random.default_rng(len(dtype) + 7 * sum(map(ord, dtype)))
    dt = np.dtype(dtype)
    if dt.kind == "b":
        return rng.random(SHAPE) < 0.5
    if dt.kind == "f":
        X = (rng.integers(0, 400, SHAPE) / 2.0).astype(dt)
        X[0, 0], X[-1, -1] = 0.0, 1024.5
        return X
    info = np.iinfo(dt)
    lo, hi = max(info.min, -2 ** 53), min(info.max, 2 ** 53)
    X = rng.integers(max(lo, -1000), min(hi, 1000), SHAPE, endpoint=True).astype(dt)
    X[0, 0], X[-1, -1], X[2, 17] = lo, hi, 0
    return X


def _device(dtype):
    import torch
    return torch.from_numpy(_host(dtype)).to("cuda")


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("dtype", list(TABLE))
def test_dtype_code_and_values_follow_the_as_measured_table(image, dtype, where):
    import torch
    host = _host(dtype)
    Xd, code, dev = image.on_device(host if where == "host" else _device(dtype))
    want = TABLE[dtype]
    assert Xd.is_cuda and Xd.device == dev and tuple(Xd.shape) == SHAPE
    assert Xd.dtype == getattr(torch, want) and code == _codes()[want]
    assert Xd.stride(1) == 1 and Xd.stride(0) >= SHAPE[1]
    got = Xd.cpu().numpy()
    assert got.dtype == np.dtype(want) and np.array_equal(got, host.astype(want))
    assert np.array_equal(got.astype(host.dtype), host)   # (the target holds every value: nothing was rounded)


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("dtype", READ_AS_THEY_ARE)
def test_a_readable_device_tensor_is_used_in_place(image, dtype, padded):
    import torch
    X = _device(dtype)
    if padded:   # a row stride above the row length
        wide = np.zeros((SHAPE[0], SHAPE[1] + 11), dtype=dtype)
        wide[:, :SHAPE[1]] = _host(dtype)
        X = torch.from_numpy(wide).to("cuda")[:, :SHAPE[1]]
        assert X.stride() == (SHAPE[1] + 11, 1)
    Xd, code, dev = image.on_device(X)
    assert Xd.data_ptr() == X.data_ptr() and Xd.stride() == X.stride() and Xd.dtype == X.dtype
    assert code == _codes()[dtype] and dev == X.device


@pytest.mark.parametrize("dtype", ["uint8", "float64", "int16"])
def test_a_transposed_view_comes_back_contiguous(image, dtype):
    import torch
    host = _host(dtype)
    X = torch.from_numpy(np.ascontiguousarray(host.T)).to("cuda").t()
    assert tuple(X.shape) == SHAPE and X.stride() == (1, SHAPE[0])
    Xd, code, _ = image.on_device(X)
    assert Xd.stride() == (SHAPE[1], 1) and Xd.is_contiguous() and code == _codes()[TABLE[dtype]]
    assert np.array_equal(Xd.cpu().numpy(), host.astype(TABLE[dtype]))


@pytest.mark.parametrize("dtype", ["uint8", "int32", "float32"])
def test_a_host_image_goes_up_in_row_chunks_in_the_dtype_it_is_read_in(image, dtype, monkeypatch):
    import torch
    host = _host(dtype)
    whole = image.on_device(host)[0]
    steps = []
    real = torch.from_numpy
    monkeypatch.setattr(torch, "from_numpy", lambda a: steps.append((a.shape, a.dtype)) or real(a))
    monkeypatch.setattr(image, "UPLOAD_ENTRIES", 80)
    Xd, code, _ = image.on_device(host)
    monkeypatch.undo()
    want = np.dtype(TABLE[dtype])
    assert steps == [((2, 37), want), ((2, 37), want), ((1, 37), want)]   # 80 // 37 = 2 rows a step, each in the dtype of the table: no wider copy
    assert Xd.dtype == whole.dtype and torch.equal(Xd, whole) and code == _codes()[TABLE[dtype]]
