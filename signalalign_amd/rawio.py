"""The raw-read file signalMachine takes in place of a .npRead (this repository reads no HDF5): one read's ADC samples, the
five channel / read attributes the event detector needs, and the basecalled sequence.  Little-endian, in this order:

    8 bytes    the magic  SARAW1\\0\\0
    5 float32  digitisation, offset, range, sampling_rate, start_time
    int64      n_samples   (1 .. 2**31 - 1)
    int64      seq_len
    seq_len    bytes of the sequence
    n_samples  int16 samples

The C loader is sa_rawread_load (csrc/sa_io.c); INTEGRATION.md shows how to write one from a fast5 with h5py.
"""
import struct

import numpy as np

MAGIC = b"SARAW1\0\0"
_HEAD = struct.Struct("<8s5fqq")


def write_raw(path, raw, digitisation, offset, range, sample_rate, start_time, sequence):
    """raw: int16 ADC counts (Raw/Reads/Read_*/Signal); the floats as the fast5's channel_id attributes and the read's
    start_time; sequence: the basecalled read (str or bytes)."""
    raw = np.ascontiguousarray(raw)
    if raw.dtype != np.int16:
        if raw.size and (raw.min() < -32768 or raw.max() > 32767):
            raise ValueError("raw samples do not fit int16")
        raw = raw.astype(np.int16)
    if raw.ndim != 1 or not 1 <= raw.size <= 2 ** 31 - 1:
        raise ValueError("a raw read holds 1 .. 2**31 - 1 samples")
    seq = sequence.encode("ascii") if isinstance(sequence, str) else bytes(sequence)
    if b"\0" in seq:
        raise ValueError("the sequence holds a NUL byte")
    with open(path, "wb") as f:
        f.write(_HEAD.pack(MAGIC, digitisation, offset, range, sample_rate, start_time, raw.size, len(seq)))
        f.write(seq)
        f.write(raw.astype("<i2", copy=False).tobytes())


def is_raw(path):
    try:
        with open(path, "rb") as f:
            return f.read(8) == MAGIC
    except OSError:
        return False


def read_raw(path):
    """dict(raw, digitisation, offset, range, sample_rate, start_time, sequence): a job of detect_events_batch /
    npread_from_raw_batch plus its sequence.  ValueError for a file the C loader refuses too."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) >= 8 and data[:8] != MAGIC:
        raise ValueError("%s: not a raw-read file (magic)" % path)
    if len(data) < _HEAD.size:
        raise ValueError("%s: truncated header" % path)
    _, dig, off, rng, rate, start, n, seq_len = _HEAD.unpack_from(data)
    if not 1 <= n <= 2 ** 31 - 1 or seq_len < 0:
        raise ValueError("%s: n_samples or seq_len out of range" % path)
    if len(data) != _HEAD.size + seq_len + 2 * n:
        raise ValueError("%s: %d bytes, the header promises %d" % (path, len(data), _HEAD.size + seq_len + 2 * n))
    seq = data[_HEAD.size:_HEAD.size + seq_len]
    raw = np.frombuffer(data, dtype="<i2", count=n, offset=_HEAD.size + seq_len).astype(np.int16)
    return dict(raw=raw, digitisation=dig, offset=off, range=rng, sample_rate=rate, start_time=start, sequence=seq.decode("ascii"))
