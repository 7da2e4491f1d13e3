"""GPU (-m gpu): `tensors.fr_from_small` against `tensors.fr_words` of the same integers, on the default stream and on a side stream; and
`buffers.DeviceBuffer`: upload at an offset, download, `free()` twice, and the `with` block left through an exception."""
import numpy as np
import pytest
import torch

from zksnap_circuits_halo2_amd import tensors as T
from zksnap_circuits_halo2_amd.buffers import DeviceBuffer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SMALL = {0: [2**63 - 1], 4: [0, 1, 2**31, 2**63 - 1] + [3 * i + 7 for i in range(12)]}      # k -> 2^k rows


@pytest.mark.parametrize("side", [False, True], ids=["default-stream", "side-stream"])
@pytest.mark.parametrize("k", sorted(SMALL))
def test_fr_from_small_equals_fr_words(lib, k, side):
    values = SMALL[k]
    assert len(values) == 1 << k
    want = T.fr_words(values, DEV)
    if side:
        stream = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(stream):                      # the input is made on the stream the program runs on
            got = T.fr_from_small(torch.tensor(values, dtype=torch.int64, device=DEV), k, stream=stream.cuda_stream)
        stream.synchronize()
    else:
        got = T.fr_from_small(torch.tensor(values, dtype=torch.int64, device=DEV), k)
        torch.cuda.synchronize()
    assert got.dtype == torch.int64 and tuple(got.shape) == (1 << k, 4) and got.device == DEV
    assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    assert T.fr_ints(got) == values


def test_device_buffer_uploads_at_an_offset_and_frees_once(lib):
    head, tail = np.arange(4, dtype=np.uint64) + 0xA0, np.array([1 << 63, 2, 3, (1 << 64) - 1], dtype=np.uint64)
    buf = DeviceBuffer(64)
    assert buf.nbytes == 64 and buf.ptr and buf.address == buf.ptr.value
    buf.upload(head)
    buf.upload(tail, offset=32)
    assert buf.download((8,)).tobytes() == head.tobytes() + tail.tobytes()
    assert buf.download((4,), offset=32).tobytes() == tail.tobytes()
    buf.free()
    assert not buf.ptr and buf.address is None
    buf.free()                                               # a second free does nothing
    assert not buf.ptr


def test_device_buffer_is_freed_when_the_with_block_raises(lib):
    with pytest.raises(RuntimeError, match="on purpose"):
        with DeviceBuffer(64) as buf:
            assert buf.ptr
            raise RuntimeError("on purpose")
    assert not buf.ptr
    with DeviceBuffer(64) as a, DeviceBuffer(64) as b:
        assert a.ptr and b.ptr and a.address != b.address
    assert not a.ptr and not b.ptr
