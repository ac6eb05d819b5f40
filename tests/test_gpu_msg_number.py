"""The device message layer's call numbering and in-kernel upload
(msg_kernels.hip k_number_one, the hipcub scan + k_chunk_base + k_call_list
it replaces, and upload_body in k_msg_init) over INJECTED state, through the
test-only harness tests/csrc/msg_stage_check.hip (number_run, upload_run),
against numpy.

End to end both run only at the sizes the message tests happen to have.  Here
the numbering gets every shape of uniq / ref / empty slots at slot counts
around the run lengths of the single workgroup (1, 2, 3 and 4 slots a
thread), both forms must agree with numpy.cumsum and with each other, and the
upload gets every tail length around its 16-byte chunks."""
import numpy as np
import pytest

from msg_stage_util import MARK8, MARK32, load_harness, ptr

pytestmark = pytest.mark.gpu

HIP_ERROR_INVALID_VALUE = 1
SLOTS = [3, 63, 1023, 1026, 2049, 4095]
PATTERNS = ["all_unique", "no_candidate", "last_only", "first_only", "random_refs", "random_empty"]


@pytest.fixture(scope="module")
def h(lib):
    h = load_harness()
    assert h.msg_stage_number_one_max() == 4096
    return h


def pattern(name, m, rng):
    """-> chash, uniq, ref for m slots (ref[c] <= c, as k_dedup_resolve leaves
    them: a repeat points at an earlier unique slot, every other slot at
    itself)."""
    has = np.ones(m, dtype=bool)
    uniq = np.ones(m, dtype=np.uint32)
    ref = np.arange(m, dtype=np.uint32)
    if name == "no_candidate":
        has[:] = False
        uniq[:] = 0
    elif name == "last_only":
        has[:-1] = False
        uniq[:-1] = 0
    elif name == "first_only":
        uniq[1:] = 0
        ref[1:] = 0
    elif name in ("random_refs", "random_empty"):
        if name == "random_empty":
            has = rng.random(m) < 0.6
        uniq = ((rng.random(m) < 0.4) & has).astype(np.uint32)
        firsts = []
        for c in range(m):
            if not has[c]:
                continue
            if uniq[c] or not firsts:
                uniq[c] = 1
                firsts.append(c)
            else:
                ref[c] = firsts[int(rng.integers(len(firsts)))]
    chash = np.where(has, rng.integers(1, 1 << 62, size=m, dtype=np.uint64) | np.uint64(1), np.uint64(0))
    return chash.astype(np.uint64), uniq, ref


def number(h, chash, uniq, ref, base, one):
    m = len(chash)
    idx, call_of = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
    cand_of = np.zeros(base + m, np.uint32)
    b1, rc = np.zeros(1, np.uint32), np.zeros(1, np.int32)
    assert h.number_run(m // 3, ptr(chash), ptr(uniq), ptr(ref), base, 1 if one else 0, ptr(idx), ptr(call_of),
                        ptr(cand_of), ptr(b1), ptr(rc)) == 0
    return idx, call_of, cand_of, int(b1[0]), int(rc[0])


@pytest.mark.parametrize("m", SLOTS)
def test_numbering_both_forms_equal_cumsum(h, m):
    rng = np.random.default_rng(m)
    for name in PATTERNS:
        chash, uniq, ref = pattern(name, m, rng)
        for base in (0, 12345):
            idx = base + np.concatenate(([0], np.cumsum(uniq)[:-1])).astype(np.int64)
            end = base + int(uniq.sum())
            call_of = np.where(chash != 0, idx[ref], MARK32)
            cand_of = np.full(base + m, MARK32, dtype=np.int64)
            cand_of[idx[uniq == 1]] = np.nonzero(uniq == 1)[0]
            for one in (True, False):
                got = number(h, chash, uniq, ref, base, one)
                assert got[4] == 0, (name, base, one)
                assert np.array_equal(got[0], idx), (name, base, one)
                assert np.array_equal(got[1], call_of), (name, base, one)
                assert np.array_equal(got[2], cand_of), (name, base, one)
                assert got[3] == end, (name, base, one)


def test_number_one_refuses_more_than_its_maximum(h):
    m = 3 * 1366  # 4,098 slots > kNumberOneMax
    chash, uniq, ref = pattern("all_unique", m, np.random.default_rng(0))
    idx, call_of, cand_of, b1, rc = number(h, chash, uniq, ref, 0, True)
    assert rc == HIP_ERROR_INVALID_VALUE
    # nothing launched: every output still holds the harness's marker
    assert (idx == MARK32).all() and (call_of == MARK32).all() and (cand_of == MARK32).all() and b1 == MARK32
    # the scan form takes the same input
    idx, _, _, b1, rc = number(h, chash, uniq, ref, 0, False)
    assert rc == 0 and b1 == m and np.array_equal(idx, np.arange(m))


@pytest.mark.parametrize("nbytes", [0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 4101, 65536 + 7])
def test_upload_copies_masks_and_zero_fills(h, nbytes):
    fill = (nbytes & ~3) + 24  # msgdev.cpp: the arena's upload
    src = np.random.default_rng(nbytes).integers(1, 256, size=max(nbytes, 1), dtype=np.uint8)[:nbytes]
    src = np.ascontiguousarray(src)
    out = np.zeros(fill + 64, dtype=np.uint8)
    assert h.upload_run(ptr(src) if nbytes else None, nbytes, fill, ptr(out)) == 0
    assert np.array_equal(out[:nbytes], src)
    assert (out[nbytes:fill] == 0).all()
    assert (out[fill:] == MARK8).all()
