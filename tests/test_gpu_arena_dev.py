"""The blocked arena reads of minbft_amd/csrc/arena_dev.h on the GPU, one
case per lane through the test-only harness tests/csrc/msg_stage_check.hip
(arena_run), against hashlib and the arena's own bytes.

End to end (tests/test_gpu_msgdev.py) a wrong sha256_arena shows only where a
valid signature exists for the message, which pins seven operation lengths;
tests/test_gpu_sha.py covers the padding boundaries of k_sha256_var, other
code.  Here every length 0..200 (and the two- and four-block boundaries
beyond) is hashed at every word alignment and at the offsets next to a
64-byte line.  Every arena exists twice, the same fields at the same offsets
between different filler, and every result must be the same for both: a read
that lets a byte outside its field through shows as a difference."""
import hashlib

import numpy as np
import pytest

from msg_stage_util import MARK8, Arena, load_harness, ptr

pytestmark = pytest.mark.gpu

SHA_LENS = list(range(201)) + [247, 248, 255, 256, 257, 1000]
SHA_MOD64 = [0, 1, 2, 3, 61, 63]  # off & 3 in 0..3, and the offsets around a 64-byte line


@pytest.fixture(scope="module")
def h(lib):
    return load_harness()


def run(h, op, arena, offs, lens, k0s=None):
    n = len(offs)
    off = np.array(offs, dtype=np.uint64)
    ln = np.array(lens, dtype=np.uint32)
    k0 = np.array(k0s if k0s is not None else [0] * n, dtype=np.uint32)
    out = np.zeros((n, 26 if op == 2 else 8), dtype=np.uint32)
    assert h.arena_run(op, ptr(arena), len(arena), ptr(off), ptr(ln), ptr(k0), n, ptr(out)) == 0
    return out


def run_both(h, op, ab, offs, lens, k0s=None):
    x, y = (run(h, op, a, offs, lens, k0s) for a in ab)
    assert np.array_equal(x, y), "the filler around the fields changed a result"
    return x


def fields(lens_aligns, mod, seed):
    """Random fields of the given (length, offset mod `mod`) -> the two arena
    copies, offsets and the fields' bytes.  Every third field follows its
    neighbour's alignment padding directly, the others keep a filler gap."""
    ar = Arena(seed)
    offs, data = [], []
    for j, (ln, al) in enumerate(lens_aligns):
        d = bytes(ar.rng.randrange(256) for _ in range(ln))
        if j % 3:
            ar._pad(1 + j % 5)
        offs.append(ar.put(d, al, mod))
        data.append(d)
    return ar.finish(), offs, data


def test_sha256_arena_lengths_and_alignments(h):
    cases = [(ln, al) for ln in SHA_LENS for al in SHA_MOD64]
    ab, offs, data = fields(cases, 64, seed=1)
    assert {o & 3 for o in offs} == {0, 1, 2, 3} and {o % 64 for o in offs} == set(SHA_MOD64)
    lens = [len(d) for d in data]
    # empty fields carry any offset inside the allocation
    nb = len(ab[0])
    for off in (0, 1, 2, 3, 63, 64, nb - 1, nb):
        offs.append(off)
        lens.append(0)
        data.append(b"")
    out = run_both(h, 0, ab, offs, lens)
    for j, d in enumerate(data):
        got = b"".join(int(w).to_bytes(4, "big") for w in out[j])
        assert got == hashlib.sha256(d).digest(), (lens[j], offs[j] % 64)


def test_sha256_arena_field_at_the_arena_end(h):
    """The last field ends with the arena: the rest of its tail word is the
    allocation's padding."""
    for ln in (1, 3, 55, 56, 64, 119, 120):
        for al in range(4):
            ar = Arena(100 + ln)
            d = bytes(ar.rng.randrange(256) for _ in range(ln))
            off = ar.put(d, al, 4)
            ab = ar.finish(tail=0)
            assert off + ln == len(ab[0])
            out = run_both(h, 0, ab, [off], [ln])
            assert b"".join(int(w).to_bytes(4, "big") for w in out[0]) == hashlib.sha256(d).digest(), (ln, al)


def test_arena_block_bytes_inside_the_field(h):
    cases = [(ln, al) for ln in range(1, 81) for al in range(4)]
    ab, offs, data = fields(cases, 4, seed=2)
    # (bytes past the field's end are unspecified: they may follow the filler,
    # so each copy is checked on its own)
    for k0 in (0, 8, 16):
        for arena in ab:
            out = run(h, 1, arena, offs, [len(d) for d in data], [k0] * len(offs))
            for j, d in enumerate(data):
                got = out[j].astype("<u4").tobytes()  # output words k0 .. k0 + 7, little-endian
                lo = 4 * k0
                inside = max(0, min(len(d) - lo, 32))
                assert got[:inside] == d[lo:lo + inside], (len(d), offs[j] & 3, k0)


def test_stage_field_fits_or_stages_nothing(h):
    cases = [(ln, al) for ln in [0, 1, 2, 3, 4] + list(range(93, 102)) for al in range(4)]
    ab, offs, data = fields(cases, 4, seed=3)
    seen = set()
    # (the slot holds the covering WORDS: its bytes before and after the field
    # follow the filler, so each copy is checked on its own)
    for arena in ab:
        out = run(h, 2, arena, offs, [len(d) for d in data])
        for j, d in enumerate(data):
            a = offs[j] & 3
            fits = len(d) > 0 and a + len(d) <= 100  # 25 words
            seen.add(fits)
            assert int(out[j][0]) == (1 if fits else 0), (len(d), a)
            slot = out[j][1:].astype("<u4").tobytes()
            if fits:
                assert slot[a:a + len(d)] == d, (len(d), a)
            else:
                assert slot == bytes([MARK8]) * 100, (len(d), a)
    assert seen == {True, False}
