"""tests/golden/small_windows.json checked on its own, without a GPU: every
expectation against the C oracle, every label against the digit property it
names under a local copy of the comb's recoding (scalar_dev.h comb_digit),
and the set of labels against the seams of the verify forms -- so that the
fixture cannot lose a case, or a case its property, unnoticed.  The GPU
tests (test_gpu_small_windows.py) run every vector of the file; none is left
out there, so nothing is left out here either.
"""
import os
import re

import pytest

from golden_util import GOLDEN, load

NAME = "small_windows.json"
WINDOWS = (4, 5, 6, 7)
N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
ROLES = ("u1", "u2", "both")


def digits(u, W):
    """comb_digit over the S = ceil(256 / W) windows of u, low to high: a
    window plus the carry above 2^(W-1) becomes negative and carries, the top
    window stays unsigned."""
    S = -(-256 // W)
    out, carry = [], 0
    for i in range(S):
        x = ((u >> (W * i)) & ((1 << W) - 1)) + carry
        neg = i + 1 < S and x > 1 << (W - 1)
        out.append(x - (1 << W) if neg else x)
        carry = 1 if neg else 0
    assert sum(d << (W * i) for i, d in enumerate(out)) == u
    return out


def range_starts(W):
    """Where a form starts a range of one scalar's windows: k_verify_split,
    the resident one-workgroup form and verify_quad at 0 and mid; the
    resident two-workgroup form at j S / 4 (split_item)."""
    S = -(-256 // W)
    return sorted({0, (S + 1) // 2} | {j * S // 4 for j in (1, 2, 3)})


def seams(W):
    """The range starts, the first window past comb_range_uniform's preload
    of 16 after each, and window 2 (after comb_start_affine's pair)."""
    S = -(-256 // W)
    st = range_starts(W)
    return sorted(set(st + [k + 16 for k in st if k + 16 < S] + [2]))


def test_seam_sets():
    assert seams(4) == [0, 2, 16, 32, 48]
    assert seams(5) == [0, 2, 13, 16, 26, 29, 39, 42]
    assert seams(6) == [0, 2, 10, 16, 21, 22, 26, 32, 37, 38]
    assert seams(7) == [0, 2, 9, 16, 18, 19, 25, 27, 34, 35]
    # the split form's ranges outgrow the preload at exactly these windows
    assert [(-(-256 // W) + 1) // 2 for W in WINDOWS] == [32, 26, 22, 19]


@pytest.fixture(scope="module")
def vectors():
    v = load(NAME)
    for x in v:
        assert sorted(x) == ["e", "expect", "label", "qx", "qy", "r", "s"]
        assert re.fullmatch(r"(any|w[4-7]):\w+(:(u1|u2|both))?(:bad)?", x["label"]), x["label"]
    return v


def _crafted(vectors):
    return [x for x in vectors if ":comb_" not in x["label"]]


def test_size_cap():
    """No larger than the largest golden file there was before it (prehashed.json)."""
    assert os.path.getsize(os.path.join(GOLDEN, NAME)) <= 224121


def test_expectations_against_the_c_oracle(vectors):
    from oracle import c_oracle
    bad = [x["label"] for x in vectors
           if c_oracle.verify(bytes.fromhex(x["qx"] + x["qy"]), bytes.fromhex(x["e"]), bytes.fromhex(x["r"]),
                              bytes.fromhex(x["s"])) != x["expect"]]
    assert not bad, bad[:10]


def test_pairs_and_half_accept(vectors):
    """An accepting vector, then the same with e ^ 1 and ":bad": half of the
    crafted (edge and seam) vectors accept.  One key for all of them."""
    c = _crafted(vectors)
    assert len(c) == 492 and len(c) % 2 == 0
    assert len({x["qx"] + x["qy"] for x in c}) == 1
    for good, bad in zip(c[0::2], c[1::2]):
        assert (good["expect"], bad["expect"]) == (1, 0), good["label"]
        assert bad["label"] == good["label"] + ":bad"
        assert int(bad["e"], 16) == int(good["e"], 16) ^ 1
        assert all(bad[k] == good[k] for k in ("qx", "qy", "r", "s"))
    assert sum(x["expect"] for x in c) * 2 == len(c)
    labels = [x["label"] for x in vectors]
    assert len(set(labels)) == len(labels)


def _holds(name, u, W):
    """The digit property `name` states, of scalar u at window W."""
    S = -(-256 // W)
    L = 256 - (S - 1) * W
    mid = (S + 1) // 2
    half = 1 << (W - 1)
    d = digits(u, W)
    raw = [(u >> (W * i)) & ((1 << W) - 1) for i in range(S)]
    if name in ("top_Nm1", "top_rnd"):
        # the carry reaches the top window: the last entry of the last table
        return d[-1] == 1 << L and N - (1 << 200) <= u < N and (name == "top_rnd" or u == N - 1)
    if name == "half":
        return d[:-1] == [half] * (S - 1)
    if name == "halfp1":
        return raw[:-1] == [half + 1] * (S - 1) and all(x < 0 for x in d[:-1])
    if name == "halfm1":
        return d[:-1] == [half - 1] * (S - 1)
    if name == "ones_carry":
        return u == (1 << 255) - 1 and d[0] == -1 and d[1:-1] == [0] * (S - 2) and d[-1] > 0
    if name in ("one", "two"):
        return u == (1 if name == "one" else 2) and d == [u] + [0] * (S - 1)
    if name == "low_only":
        return u < 1 << (W * mid) and d[mid:] == [0] * (S - mid) and any(d[:mid])
    if name == "high_only":
        return u % (1 << (W * mid)) == 0 and d[:mid] == [0] * mid and any(d[mid:])
    m = re.fullmatch(r"seam(\d+)_(carry|half|z0|z01|z1)", name)
    k, kind = int(m.group(1)), m.group(2)
    if kind == "carry":  # all-ones windows below k, and their carry arrives in window k
        return raw[k - 1] == (1 << W) - 1 and d[k - 1] <= 0 and d[k] == raw[k] + 1
    if kind == "half":
        return d[k - 1] == half and d[k] == half
    return [d[k] == 0, d[k + 1] == 0] == {"z0": [True, False], "z01": [True, True], "z1": [False, True]}[kind]


def test_every_label_keeps_its_property(vectors):
    for x in _crafted(vectors):
        if not x["expect"]:
            continue
        prefix, name, role = x["label"].split(":")
        w = pow(int(x["s"], 16), -1, N)
        u1, u2 = int(x["e"], 16) * w % N, int(x["r"], 16) * w % N
        for W in (WINDOWS if prefix == "any" else (int(prefix[1:]),)):
            for u in {"u1": (u1,), "u2": (u2,), "both": (u1, u2)}[role]:
                assert _holds(name, u, W), (x["label"], W)


def test_every_case_of_every_window_is_there(vectors):
    """Nothing of the cross product the generator's docstring states is
    missing: the cap on left-out cases is zero."""
    have = {x["label"] for x in vectors}
    want = {"any:top_Nm1:" + r for r in ROLES} | {"any:%s:u2" % n for n in ("ones_carry", "one", "two")}
    for W in WINDOWS:
        S = -(-256 // W)
        mid = (S + 1) // 2
        p = "w%d:" % W
        want |= {p + n + ":" + r for n in ("top_rnd", "half") for r in ROLES}
        want |= {p + n + ":u2" for n in ("halfp1", "halfm1", "low_only", "high_only")}
        for k in seams(W):
            want |= {p + "seam%d_%s:u2" % (k, z) for z in ("z0", "z01")}
            if k in range_starts(W):
                want.add(p + "seam%d_z1:u2" % k)
            if k > 0:
                want |= {p + "seam%d_carry:%s" % (k, r) for r in ROLES}
                want.add(p + "seam%d_half:u2" % k)
        for i in (0, 1, 2, mid - 1, mid, S - 2, S - 1):
            want.add(p + "comb_dbl%d" % i)
            if i < S - 1:
                want.add(p + "comb_inf%d" % i)
    want |= {l + ":bad" for l in want if ":comb_" not in l}
    assert have == want, (sorted(want - have)[:10], sorted(have - want)[:10])
    assert len(want) == 544


def test_collisions_collide(vectors):
    """w<W>:comb_dbl<i> / comb_inf<i>: with the W-bit recoding of u2, the
    accumulator before window i -- u1 G plus Q's windows below i -- is the
    window's addend (a doubling) or its negative (the sum is infinity)."""
    from oracle import p256 as o
    n = 0
    for x in vectors:
        m = re.fullmatch(r"w(\d):comb_(dbl|inf)(\d+)", x["label"])
        if not m:
            continue
        n += 1
        W, kind, i = int(m.group(1)), m.group(2), int(m.group(3))
        assert x["expect"] == 1
        q = (int(x["qx"], 16), int(x["qy"], 16))
        w = pow(int(x["s"], 16), -1, N)
        u1, u2 = int(x["e"], 16) * w % N, int(x["r"], 16) * w % N
        d = digits(u2, W)
        assert d[i] != 0, x["label"]
        partial = sum(v << (W * j) for j, v in enumerate(d[:i])) % N
        acc = o.scalar_mult(u1, o.G)
        if partial:
            acc = o.point_add(acc, o.scalar_mult(partial, q))
        addend = o.scalar_mult((d[i] << (W * i)) % N, q)
        assert acc == (addend if kind == "dbl" else o.point_neg(addend)), x["label"]
    assert n == 52
