"""halo2's `Blake2bWrite` / `Blake2bRead` with `Challenge255` [DEP halo2-axiom transcript.rs] over the C ABI (include/zkhip.h, "transcript"):
what joins `create_proof` and `verify_proof` into a proof that exists as bytes.  The benches prove with `create_proof(SHPLONK, Blake2b)`
(halo2-base `gen_proof`, /root/reference/aggregator/benches/wrapper_circuit.rs:140).

The hash, the framing and the challenge reduction live in libzkhip.so (host code); the device does the curve and field work that feeds the
hash: `write_points` takes Jacobian commitments as the MSM calls leave them in HBM, `write_scalars` a device buffer of Montgomery Fr, and
`read_points` leaves affine Montgomery points in HBM for the verifier's MSMs.  Scalars cross this interface as Python integers (canonical),
points as (n, 12) / (n, 8) arrays of uint64 limbs or torch tensors on the device; nothing here computes: there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import hashlib
from typing import List, Sequence

import numpy as np

from . import _lib
from .fields import R_MOD, fr_decode, fr_encode
from .tensors import stream_of


def _is_device(x) -> bool:
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


class _Transcript:
    def __init__(self, handle):
        if not handle:
            raise _lib.ZkhipError(-1, _lib.load().zkhip_last_error().decode(errors="replace"))
        self._lib, self._t = _lib.load(), C.c_void_p(handle)

    def close(self) -> None:
        if self._t is not None:
            self._lib.zkhip_transcript_free(self._t)
            self._t = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- TranscriptRead / TranscriptWrite's common part ------------------------------------------------------------------------------------
    def common_scalar(self, s: int) -> None:
        w = fr_encode([s])
        _lib.check(self._lib.zkhip_transcript_common_scalars(self._t, w.ctypes.data, 1))

    def common_scalars(self, scalars: Sequence[int]) -> None:
        w = fr_encode(list(scalars))
        _lib.check(self._lib.zkhip_transcript_common_scalars(self._t, w.ctypes.data, len(w)))

    def common_point(self, affine) -> None:
        """`affine`: 8 uint64 limbs (x | y, Montgomery: the memory of `G1Affine`); the identity is refused"""
        w = np.ascontiguousarray(affine, dtype=np.uint64).reshape(-1, 8)
        _lib.check(self._lib.zkhip_transcript_common_points(self._t, w.ctypes.data, len(w)))

    def squeeze_challenge(self) -> int:
        out = np.zeros(4, dtype=np.uint64)
        _lib.check(self._lib.zkhip_transcript_squeeze(self._t, out.ctypes.data))
        return fr_decode(out.reshape(1, 4))[0]

    def proof(self) -> bytes:
        n = C.c_size_t(0)
        _lib.check(self._lib.zkhip_transcript_proof(self._t, None, 0, C.byref(n)))
        buf = C.create_string_buffer(max(n.value, 1))
        _lib.check(self._lib.zkhip_transcript_proof(self._t, buf, n.value, C.byref(n)))
        return buf.raw[:n.value]


class _Write(_Transcript):
    """the writing calls: the library dispatches on the object's hash, the proof bytes are the same under either"""

    def write_points(self, points, stream=None) -> None:
        """Jacobian commitments, 12 limbs each: a torch tensor on the device (one launch, one copy, one wait on `stream`) or host limbs"""
        if _is_device(points):
            n = points.numel() // 12
            _lib.check(self._lib.zkhip_transcript_write_points_device(self._t, points.data_ptr(), n, stream_of(stream)))
        else:
            w = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 12)
            _lib.check(self._lib.zkhip_transcript_write_points(self._t, w.ctypes.data, len(w)))

    def write_scalars(self, scalars, stream=None) -> None:
        """a torch tensor of Montgomery Fr on the device (4 limbs each), or Python integers"""
        if _is_device(scalars):
            _lib.check(self._lib.zkhip_transcript_write_scalars_device(self._t, scalars.data_ptr(), scalars.numel() // 4, stream_of(stream)))
        else:
            w = fr_encode([int(s) for s in scalars])
            _lib.check(self._lib.zkhip_transcript_write_scalars(self._t, w.ctypes.data, len(w)))

    def write_scalar(self, s: int) -> None:
        self.write_scalars([s])

    def finalize(self) -> bytes:
        return self.proof()


class _Read(_Transcript):
    def read_points(self, n: int, device: bool = True, stream=None):
        """n points -> affine Montgomery limbs: an (n, 8) int64 torch tensor on the device, or with device=False an (n, 8) uint64 array.  A bad
        encoding raises ZkhipError (ZKHIP_EINVAL) and leaves the transcript where it was."""
        if device:
            import torch

            out = torch.empty((n, 8), dtype=torch.int64, device="cuda")
            _lib.check(self._lib.zkhip_transcript_read_points_device(self._t, n, out.data_ptr(), stream_of(stream)))
            return out
        out = np.zeros((n, 8), dtype=np.uint64)
        _lib.check(self._lib.zkhip_transcript_read_points(self._t, n, out.ctypes.data))
        return out

    def read_scalars(self, n: int) -> List[int]:
        out = np.zeros((n, 4), dtype=np.uint64)
        _lib.check(self._lib.zkhip_transcript_read_scalars(self._t, n, out.ctypes.data))
        return fr_decode(out)

    def read_scalar(self) -> int:
        return self.read_scalars(1)[0]


class Blake2bWrite(_Write):
    """`Blake2bWrite::<_, G1Affine, Challenge255<_>>::init(vec![])`; `finalize()` returns the proof"""

    def __init__(self, flag_layout: int = 0):
        super().__init__(_lib.load().zkhip_transcript_new(flag_layout))


class Blake2bRead(_Read):
    """`Blake2bRead::<_, G1Affine, Challenge255<_>>::init(proof)`"""

    def __init__(self, proof: bytes, flag_layout: int = 0):
        proof = bytes(proof)
        super().__init__(_lib.load().zkhip_transcript_new_reader(proof, len(proof), flag_layout))


class PoseidonWrite(_Write):
    """snark-verifier's `PoseidonTranscript::<G1Affine, NativeLoader, _>::new(vec![])`, the transcript of the reference's `gen_snark`
    (include/zkhip.h, "Poseidon"): the same calls and the same proof bytes as `Blake2bWrite`, other challenges"""

    def __init__(self, flag_layout: int = 0):
        super().__init__(_lib.load().zkhip_transcript_new_poseidon(flag_layout))


class PoseidonRead(_Read):
    def __init__(self, proof: bytes, flag_layout: int = 0):
        proof = bytes(proof)
        super().__init__(_lib.load().zkhip_transcript_new_poseidon_reader(proof, len(proof), flag_layout))


WRITERS = {"blake2b": Blake2bWrite, "poseidon": PoseidonWrite}
READERS = {"blake2b": Blake2bRead, "poseidon": PoseidonRead}


def transcript_classes(hash: str):
    """(writer, reader) of a hash name; ValueError on any other name"""
    if hash not in WRITERS:
        raise ValueError(f"transcript hash {hash!r}: 'blake2b' or 'poseidon'")
    return WRITERS[hash], READERS[hash]


def decoded(read, *args, **kw):
    """read(*args, **kw), or None where a reader's bytes do not decode (ZkhipError with ZKHIP_EINVAL, -1): such bytes reject one proof, the
    caller's and no other; every other error of the library passes through.  The reader is left where the failing read left it."""
    try:
        return read(*args, **kw)
    except _lib.ZkhipError as e:
        if e.code != -1:
            raise
        return None


def vk_transcript_repr(vk_bytes: bytes) -> int:
    """The scalar a proof's transcript starts with.  halo2's value hashes the `Debug` string of the pinned verifying key, which cannot be
    restated outside Rust; this is a documented STAND-IN that a Rust host replaces with the crate's own `vk.transcript_repr`: Blake2b-512,
    personalised "Halo2-Verify-Key", over the bytes `keygen.py` writes for the verifying key, reduced like a challenge."""
    return int.from_bytes(hashlib.blake2b(vk_bytes, digest_size=64, person=b"Halo2-Verify-Key").digest(), "little") % R_MOD
