"""The transcript format of include/zkhip.h restated with hashlib, for the transcript tests: the independent side of every comparison."""
import hashlib

from oracle import bn254 as O

R = O.R_MOD
Q = O.Q_MOD


def encode_point(P, layout):
    """the 32-byte GroupEncoding of an affine point (x, y), not the identity"""
    x, y = P
    b = bytearray(x.to_bytes(32, "little"))
    b[31] |= (y & 1) << (6 if layout == 0 else 7)
    return bytes(b)


class RefTranscript:
    def __init__(self, layout=0):
        self.h = hashlib.blake2b(digest_size=64, person=b"Halo2-Transcript")
        self.layout = layout
        self.proof = b""
        self.absorbed = 0

    def _update(self, data):
        self.h.update(data)
        self.absorbed += len(data)

    def common_scalar(self, s):
        self._update(b"\x02" + (s % R).to_bytes(32, "little"))

    def common_point(self, P):
        self._update(b"\x01" + P[0].to_bytes(32, "little") + P[1].to_bytes(32, "little"))

    def write_scalar(self, s):
        self.common_scalar(s)
        self.proof += (s % R).to_bytes(32, "little")

    def write_point(self, P):
        self.common_point(P)
        self.proof += encode_point(P, self.layout)

    def squeeze(self):
        self._update(b"\x00")
        return int.from_bytes(self.h.copy().digest(), "little") % R
