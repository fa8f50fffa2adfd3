"""NumPy restatement of vbnn_digest (include/vbnn_hip.h): over a buffer's 32-bit words w_i,
    digest = sum_i mix(((index0 + i + 1) << 32) | w_i)  mod 2^64,   mix = the splitmix64 finaliser.
`digest` is the vectorised uint64 form the GPU tests compare with; `digest_py` is the same definition written word by word with
Python integers (masked to 64 bits by hand), which tests/test_checkpoint_ref.py holds the first against."""
import numpy as np

M64 = (1 << 64) - 1
C1, C2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
MAX_POS = (1 << 32) - 1


def words(buf):
    """The little-endian 32-bit words of an array (any dtype whose bytes are a multiple of 4) or of a bytes object."""
    if isinstance(buf, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(buf), dtype="<u4")
    a = np.ascontiguousarray(buf)
    return a.reshape(-1).view(np.uint8).view("<u4")


def mix(z):
    z = z.astype(np.uint64, copy=True)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(C1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(C2)
        return z ^ (z >> np.uint64(31))


def digest(buf, index0=0):
    w = words(buf).astype(np.uint64)
    if index0 + w.size > MAX_POS:
        raise ValueError("index0 + n_words > 2^32 - 1")
    pos = np.arange(index0 + 1, index0 + 1 + w.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int(np.add.reduce(mix((pos << np.uint64(32)) | w), dtype=np.uint64)) & M64


def mix_py(z):
    z = ((z ^ (z >> 30)) * C1) & M64
    z = ((z ^ (z >> 27)) * C2) & M64
    return z ^ (z >> 31)


def digest_py(buf, index0=0):
    total = 0
    for i, w in enumerate(words(buf).tolist()):
        total = (total + mix_py(((index0 + i + 1) << 32) | int(w))) & M64
    return total
