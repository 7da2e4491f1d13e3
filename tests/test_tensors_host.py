"""tensors.py on the host: every conversion byte for byte against `fields.fr_encode` / `fields.fr_decode` or `int.to_bytes`, on device="cpu";
what `plume.encode_points` and `paillier.encode` returned before they shared it, as literals; and that tensors.py and buffers.py import where
there is no torch."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from zksnap_circuits_halo2_amd import fields as F, paillier, plume, tensors as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = F.R_MOD
FR_VALUES = [0, 1, R - 1, R, R + 1, 2**256 - 1]          # the last three are reduced mod r
WORDS = [3, 4, 6]


def raw(values, words):
    """flat integers -> their little-endian bytes, `words` 64-bit words each"""
    return b"".join(int(v).to_bytes(8 * words, "little") for v in values)


def test_fr_words_equals_fr_encode_and_fr_ints_inverts_it():
    t = T.fr_words(FR_VALUES, device="cpu")
    assert t.dtype == torch.int64 and tuple(t.shape) == (len(FR_VALUES), 4) and t.device.type == "cpu"
    assert t.numpy().tobytes() == F.fr_encode(FR_VALUES).tobytes()
    assert T.fr_ints(t) == F.fr_decode(F.fr_encode(FR_VALUES)) == [v % R for v in FR_VALUES]
    assert T.fr_ints(F.fr_encode(FR_VALUES)) == [v % R for v in FR_VALUES]          # an array as well as a tensor
    for v in FR_VALUES:
        one = T.fr_words([v], device="cpu")
        assert one.numpy().tobytes() == F.fr_encode([v]).tobytes() and T.fr_ints(one) == [v % R]


def test_fr_words_of_nothing():
    t = T.fr_words([], device="cpu")
    assert tuple(t.shape) == (0, 4) and t.dtype == torch.int64
    assert T.fr_ints(t) == []


def test_fr_empty_and_fr_random_on_the_host():
    assert tuple(T.fr_empty(3, 2, device="cpu").shape) == (3, 2, 4) and T.fr_empty(0, device="cpu").dtype == torch.int64
    a = T.fr_random(64, device="cpu")
    assert tuple(a.shape) == (64, 4) and a.dtype == torch.int64
    assert all(0 <= w < 1 << 61 for w in a[:, 3].tolist())                            # the top word keeps every value below 2^253 < r


@pytest.mark.parametrize("words", WORDS)
def test_to_words_and_from_words(words):
    top = (1 << (64 * words)) - 1
    scalar = 0x0123456789ABCDEF << (64 * (words - 1)) | 0xFEDC
    a = T.to_words(scalar, words)
    assert a.dtype == np.uint64 and a.shape == (words,) and a.tobytes() == raw([scalar], words) and T.from_words(a) == scalar
    flat = [0, 1, scalar, top]                                                         # the largest value among them
    a = T.to_words(flat, words)
    assert a.shape == (4, words) and a.tobytes() == raw(flat, words) and T.from_words(a) == flat
    nest = [[1, top, 1 << 63], [scalar, 0, (1 << 64) + 2]]
    a = T.to_words(nest, words)
    assert a.shape == (2, 3, words) and a.tobytes() == raw(nest[0] + nest[1], words) and T.from_words(a) == nest
    a = T.to_words([], words)
    assert a.shape == (0, words) and a.dtype == np.uint64 and T.from_words(a) == []
    t = T.raw_tensor(nest, words, device="cpu")
    assert t.dtype == torch.int64 and tuple(t.shape) == (2, 3, words) and t.numpy().tobytes() == raw(nest[0] + nest[1], words)
    assert T.from_words(t) == nest


@pytest.mark.parametrize("words", WORDS)
def test_to_words_refuses_what_does_not_fit(words):
    for bad in (1 << (64 * words), -1, [0, 1 << (64 * words)], [[1, -1]]):
        with pytest.raises(ValueError, match=rf"an integer outside \[0, 2\^{64 * words}\)"):
            T.to_words(bad, words)
    for ragged in ([[1, 2], [3]], [[1], [2, 3]], [[[1]], [[2], [3]]]):
        with pytest.raises(ValueError, match="ragged"):
            T.to_words(ragged, words)


@pytest.mark.parametrize("words", WORDS)
def test_a_word_with_bit_63_set_round_trips_through_int64(words):
    values = [1 << 63, ((1 << 63) | 5) << (64 * (words - 1)), (1 << (64 * words)) - 1]
    t = T.raw_tensor(values, words, device="cpu")
    assert t.dtype == torch.int64 and int(t[0, 0]) == -(1 << 63) and int(t[1, words - 1]) < 0 and t[2].tolist() == [-1] * words
    assert t.numpy().tobytes() == raw(values, words)
    assert T.from_words(t) == values and T.from_words(t.numpy()) == values


def test_stream_of_and_device_of():
    assert T.stream_of(None) == 0 and T.stream_of(0) == 0 and T.stream_of(0x7F00DEAD0000) == 0x7F00DEAD0000
    assert T.device_of("cpu") == torch.device("cpu") and T.device_of("cuda:1") == torch.device("cuda", 1)
    assert T.device_of(torch.device("cuda", 0)) == torch.device("cuda", 0)


# what the parent commit's plume.encode_points / paillier.encode returned for these inputs (recorded from a run of it), as int64 words
POINT = (0x0123456789ABCDEF_FEDCBA9876543210_0F1E2D3C4B5A6978_8796A5B4C3D2E1F0, 2**256 - 1)
POINT_WORDS = [[-8676565436284608016, 1089357896855742840, -81985529216486896, 81985529216486895, -1, -1, -1, -1]]
CIPHERTEXTS = [[1, 2**383 + 5], [2**64, 2**384 - 1]]
CIPHERTEXT_WORDS = [[[1, 0, 0, 0, 0, 0], [5, 0, 0, 0, 0, -9223372036854775808]], [[0, 1, 0, 0, 0, 0], [-1, -1, -1, -1, -1, -1]]]


def test_plume_and_paillier_encode_as_before():
    t = plume.encode_points([POINT], device="cpu")
    assert t.dtype == torch.int64 and tuple(t.shape) == (1, 8) and t.tolist() == POINT_WORDS
    assert t.numpy().tobytes() == raw(POINT, 4)
    assert plume.decode_points(t) == [POINT] and plume.decode_scalars(t.reshape(2, 4)) == list(POINT)
    s = plume.encode_scalars([5, 2**255], device="cpu")
    assert s.tolist() == [[5, 0, 0, 0], [0, 0, 0, -9223372036854775808]] and plume.decode_scalars(s) == [5, 2**255]
    assert tuple(plume.encode_points([], device="cpu").shape) == (0, 8) and tuple(plume.encode_scalars([], device="cpu").shape) == (0, 4)
    with pytest.raises(ValueError, match=r"an integer outside \[0, 2\^256\)"):
        plume.encode_scalars([1 << 256], device="cpu")
    with pytest.raises(ValueError, match=r"a point is a pair \(x, y\)"):
        plume.encode_points([(1, 2, 3)], device="cpu")
    u = paillier.encode(CIPHERTEXTS, device="cpu")
    assert u.dtype == torch.int64 and tuple(u.shape) == (2, 2, 6) and u.tolist() == CIPHERTEXT_WORDS
    assert u.numpy().tobytes() == raw(CIPHERTEXTS[0] + CIPHERTEXTS[1], 6)
    assert paillier.decode(u) == CIPHERTEXTS
    assert tuple(paillier.encode_exponents([[7]], device="cpu").shape) == (1, 1, 4) and tuple(paillier.encode_randomness([7], device="cpu").shape) == (1, 3)
    with pytest.raises(ValueError, match=r"an integer outside \[0, 2\^384\)"):
        paillier.encode([1 << 384], device="cpu")


def test_tensors_and_buffers_import_without_torch():
    """a fresh interpreter in which `import torch` fails: both modules import, and the conversions that need no tensor work"""
    code = ("import sys; sys.modules['torch'] = None\n"
            "import zksnap_circuits_halo2_amd.tensors as T, zksnap_circuits_halo2_amd.buffers as B\n"
            "assert T.from_words(T.to_words([[1, 2**191]], 3)) == [[1, 2**191]] and B.DeviceBuffer\n"
            "try:\n    import torch\nexcept ImportError:\n    print('no torch, both imported')\n")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "no torch, both imported", done.stderr
