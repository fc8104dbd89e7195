"""The container of a chain's checkpoint blob (hmcmt_chain_save), written and read in numpy from the text of include/hmcmt.h alone:
the 64-byte header, the section table, the payloads in table order, the FNV-style checksum over the 8-byte words -- and the payload
of CHAN, the one section whose fields the header fixes for readers outside the library.  Nothing here calls the library."""
import struct

import numpy as np

MAGIC = b"HMCMTCK\0"
TAGS = ("CHAN", "MASS", "HIST", "DMOM", "ACOV", "COV ", "ADPT", "ADLR")
MASK = (1 << 64) - 1


def checksum(body):
    """h = 0xcbf29ce484222325; for every 8-byte word w: h = (h ^ w) * 0x100000001b3 mod 2^64 -- in Python integers"""
    assert len(body) % 8 == 0
    h = 0xcbf29ce484222325
    for w in np.frombuffer(bytes(body), dtype="<u8").tolist():
        h = ((h ^ w) * 0x100000001b3) & MASK
    return h


def tag_code(tag):
    return struct.unpack("<I", tag.encode("ascii"))[0]


def write(sections, nAC, nData, mass_kind=0, seeded=0, nsamples=0, nmoments=0, version=1, table=None, total=None):
    """A blob of `sections` = [(tag, payload bytes)].  table: [(tag, offset, bytes)] written in place of the consistent one (the
    payloads still follow each other), total: the header's total in place of the true one -- for blobs that must be refused.  The
    checksum is always the true one of what precedes it."""
    n = len(sections)
    at = 64 + 24 * n
    entries = []
    for tag, payload in sections:
        assert len(payload) % 8 == 0
        entries.append((tag, at, len(payload)))
        at += len(payload)
    size = at + 8
    head = MAGIC + struct.pack("<IIQqqiIqq", version, n, size if total is None else total, nAC, nData, mass_kind, seeded, nsamples, nmoments)
    assert len(head) == 64
    body = head + b"".join(struct.pack("<IIQQ", tag_code(t), 0, o, b) for t, o, b in (entries if table is None else table))
    body += b"".join(bytes(p) for _, p in sections)
    return np.frombuffer(body + struct.pack("<Q", checksum(body)), dtype=np.uint8).copy()


def chan_payload(nAC, nData, dt=0.02, regParam=1.0, lo=-9.0, hi=0.0, D=3.0, M=0.5, burnin=0, nsamples=0, nmoments=0, seed=0, t=0, stream=0,
                 seeded=0, m=None, pred=None, mean=None, m2=None):
    arrays = [np.zeros(nAC) if m is None else m, np.zeros(2 * nData) if pred is None else pred, np.zeros(nAC) if mean is None else mean,
              np.zeros(nAC) if m2 is None else m2]
    return struct.pack("<6d3q2Q2I", dt, regParam, lo, hi, D, M, burnin, nsamples, nmoments, seed, t, stream, seeded) + \
        b"".join(np.ascontiguousarray(a, dtype="<f8").tobytes() for a in arrays)


def mass_payload(nAC, invM=None):
    """the diagonal mass: kind 0, rank 0, no low-rank buffers, no given scales; invM[nAC]"""
    return struct.pack("<4q", 0, 0, 0, 0) + np.ascontiguousarray(np.ones(nAC) if invM is None else invM, dtype="<f8").tobytes()


def read(blob):
    """{header fields, "sections": {tag: payload bytes}, "order": [tags]}; AssertionError where the container is not consistent"""
    b = bytes(np.asarray(blob, dtype=np.uint8))
    assert len(b) >= 64 + 8 and len(b) % 8 == 0 and b[:8] == MAGIC
    version, n, total, nAC, nData, kind, seeded, nsamples, nmoments = struct.unpack("<IIQqqiIqq", b[8:64])
    assert version == 1 and total == len(b)
    assert struct.unpack("<Q", b[-8:])[0] == checksum(b[:-8])
    out = {"version": version, "total_bytes": total, "nAC": nAC, "nData": nData, "mass_kind": kind, "seeded": seeded, "nsamples": nsamples,
           "nmoments": nmoments, "sections": {}, "order": []}
    at = 64 + 24 * n
    for k in range(n):
        tag, zero, off, nb = struct.unpack("<IIQQ", b[64 + 24 * k:88 + 24 * k])
        name = struct.pack("<I", tag).decode("ascii")
        assert zero == 0 and off == at and off % 8 == 0 and nb % 8 == 0 and name in TAGS and name not in out["sections"]
        out["sections"][name] = b[off:off + nb]
        out["order"].append(name)
        at += nb
    assert at + 8 == len(b)
    return out


def read_chan(payload, nAC, nData):
    """CHAN's fields as a dict, its four arrays as float64"""
    keys = ("dt", "regParam", "lo", "hi", "D", "M", "burnin", "nsamples", "nmoments", "seed", "t", "stream", "seeded")
    out = dict(zip(keys, struct.unpack("<6d3q2Q2I", payload[:96])))
    a = np.frombuffer(payload[96:], dtype="<f8")
    assert len(a) == 3 * nAC + 2 * nData
    out["m"], out["pred"], out["mean"], out["m2"] = a[:nAC], a[nAC:nAC + 2 * nData], a[nAC + 2 * nData:2 * nAC + 2 * nData], a[2 * nAC + 2 * nData:]
    return out
