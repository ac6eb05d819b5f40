"""k_verify_p384's second and later grid-stride passes: the
kernel launched under hand-made plans through tests/libp384_check.so -- 1,000
items on a one-block and a three-block grid -- and once on the product's own
grid at one full grid plus 300 items.  The items are the fixture's prehashed
vectors tiled with numpy, every 7th `s` corrupted, so the expected statuses
follow from the fixtures: a corrupted s under a valid key and a valid r turns
an accepted item into a rejected one and leaves every other status alone."""
import ctypes

import numpy as np
import pytest

import p384_ops_util as u

pytestmark = pytest.mark.gpu

ACCEPT, REJECT, BAD_KEY = 0, 1, 5
POISON = 0xEE


@pytest.fixture(scope="module")
def harness(lib):
    import __graft_entry__ as ge
    h = ctypes.CDLL(ge.build_p384_check())
    h.p384_check_launch.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    h.p384_check_launch.restype = ctypes.c_int
    h.p384_check_plan_blocks.argtypes = [ctypes.c_long]
    h.p384_check_plan_blocks.restype = ctypes.c_long
    return h


@pytest.fixture(scope="module")
def base():
    pre = [v for v in u.fixtures() if v["kind"] == "prehashed"]
    rows = lambda k: np.array([list(bytes.fromhex(v[k])) for v in pre], dtype=np.uint8)  # noqa: E731
    e, r, s = rows("e"), rows("r"), rows("s")
    xy = np.concatenate([rows("x"), rows("y")], axis=1)
    want = np.array([v["status"] for v in pre], dtype=np.uint8)
    return e, r, s, xy, want


def tiled(base, n):
    """n items: the vectors tiled, every 7th s with its low byte changed."""
    e, r, s, xy, want = base
    idx = np.arange(n) % len(want)
    e, r, s, xy, want = e[idx], r[idx], s[idx].copy(), xy[idx], want[idx].copy()
    hit = np.arange(n) % 7 == 3
    s[hit, 47] ^= 0x5A
    # an accepted item no longer verifies (s moved by less than 2^8: still in [1, N) -- checked below);
    # a rejected or bad-key item keeps its status unless the change repaired it, which one byte cannot
    # do for a rejected vector of this set (their r or key is wrong, or s is 0, N, N - 1 or 2^384 - 1)
    sv = [int.from_bytes(bytes(row), "big") for row in s[hit & (want == ACCEPT)]]
    assert all(0 < v < u.N for v in sv)
    want[hit & (want == ACCEPT)] = REJECT
    return e, r, s, xy, want, hit


def launch(h, e, r, s, xy, blocks):
    import torch
    n = len(e)
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (e, r, s, xy)]
    st = torch.full((n + 256,), POISON, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rc = h.p384_check_launch(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, st.data_ptr(),
                             blocks, None)
    assert rc == 0, rc
    out = st.cpu().numpy()
    assert (out[n:] == POISON).all()
    return out[:n]


def check(got, want, hit, what):
    bad = np.nonzero(got != want)[0]
    assert not len(bad), (what, len(bad), [(int(i), int(got[i]), int(want[i]), bool(hit[i])) for i in bad[:10]])


@pytest.mark.parametrize("blocks", [1, 3])
def test_passes_on_small_grids(harness, base, blocks):
    """1,000 items: four passes of one block (the last with 232 lanes live),
    two of three blocks (the second with 232 of 768)."""
    e, r, s, xy, want, hit = tiled(base, 1000)
    assert hit.sum() > 100 and (want[hit] != ACCEPT).all() and (want == ACCEPT).sum() > 300
    check(launch(harness, e, r, s, xy, blocks), want, hit, blocks)


def test_second_pass_on_the_products_grid(harness, base, auth_p384):
    """One full grid plus 300 items through the library's own plan: the second
    pass has 300 live lanes spread over two blocks."""
    grid = harness.p384_check_plan_blocks(1 << 24)  # the cap: blocks per CU times CUs
    assert 1 <= grid <= 4096
    n = grid * 256 + 300
    assert harness.p384_check_plan_blocks(n) == grid
    e, r, s, xy, want, hit = tiled(base, n)
    import torch
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (e, r, s, xy)]
    st = torch.full((n + 256,), POISON, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    auth_p384.verify_prehashed_p384_keys_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n,
                                                st.data_ptr(), 0)
    torch.cuda.synchronize()
    out = st.cpu().numpy()
    assert (out[n:] == POISON).all()
    check(out[:n], want, hit, "product grid")


@pytest.fixture(scope="module")
def auth_p384(lib):
    from minbft_amd.authenticator import Authenticator
    a = Authenticator(0)
    yield a
    a.close()
