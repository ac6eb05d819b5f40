"""The verified-call memo's plan (minbft_amd/csrc/memo_plan.h): the table's
shape from a byte budget, the hash, the bucket, the tag and the probe
sequence, the rotation rule, one pass's scratch, and the memo flag of the
launch plan (verify_plan.h) -- all plain C++, driven through the stand-alone
program tests/memo_plan_check (built by __graft_entry__.build() from
tests/csrc/memo_plan_check.cpp) and compared with restatements written here.
No GPU."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "memo_plan_check.cpp")
HIPCC = "/opt/rocm/bin/hipcc"
M64 = (1 << 64) - 1

ENTRY_BYTES, MIN_ENTRIES, TUPLE_WORDS = 128, 1024, 25


@pytest.fixture(scope="module")
def prog():
    import __graft_entry__ as ge
    return ge.build_memo_check_host()


def run(prog, lines):
    p = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return p.stdout.split("\n")[:-1]


def geometry(nbytes):
    """Two generations, each the largest power of two of 128-byte entries that
    fits half the budget; below 2 x 1,024 entries nothing."""
    per_gen = nbytes // (2 * ENTRY_BYTES)
    if per_gen < MIN_ENTRIES:
        return 0, 0
    e = 1 << (per_gen.bit_length() - 1)
    return e, 2 * e * ENTRY_BYTES


def memo_hash(words):
    """A multiply-rotate per word, then murmur3's 64-bit finalizer."""
    h = 0x243F6A8885A308D3
    for w in words:
        h ^= w
        h = (h * 0x9E3779B97F4A7C15) & M64
        h = ((h << 27) | (h >> 37)) & M64
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & M64
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & M64
    h ^= h >> 33
    return h


def tag_of(h):
    return ((h >> 32) | 2) & 0xFFFFFFFF


def probe_steps(prog):
    return int(run(prog, ["consts"])[0].split()[2])


def test_consts(prog):
    eb, ew, probe, mn, tw, empty, busy = (int(x) for x in run(prog, ["consts"])[0].split())
    assert (eb, ew, mn, tw, empty, busy) == (ENTRY_BYTES, 32, MIN_ENTRIES, TUPLE_WORDS, 0, 1)
    assert probe in (4, 8)


def test_geometry(prog):
    rng = random.Random(11)
    low = 2 * MIN_ENTRIES * ENTRY_BYTES
    budgets = [0, 1, 127, low - 1, low, low + 1, 2 * low - 1, 2 * low, 3 * low, 1 << 40, (1 << 40) - 1, (1 << 40) + 12345]
    budgets += [rng.randrange(0, 1 << 41) for _ in range(300)]
    budgets += [rng.randrange(0, 4 * low) for _ in range(100)]
    budgets += [(1 << k) + d for k in range(10, 41) for d in (-1, 0, 1)]
    out = run(prog, [f"geometry {b}" for b in budgets])
    for b, o in zip(budgets, out):
        e, nb = (int(x) for x in o.split())
        assert (e, nb) == geometry(b), b
        if e:
            assert e & (e - 1) == 0 and e >= MIN_ENTRIES and nb <= b < 2 * nb
    assert geometry(low - 1) == (0, 0) and geometry(low) == (MIN_ENTRIES, low)
    assert geometry(1 << 40) == (1 << 32, 1 << 40)


def test_hash_bucket_and_tag(prog):
    rng = random.Random(12)
    tuples = [[rng.randrange(1 << 32) for _ in range(TUPLE_WORDS)] for _ in range(200)]
    tuples += [[0] * TUPLE_WORDS, [0xFFFFFFFF] * TUPLE_WORDS]
    out = run(prog, ["hash " + " ".join(map(str, t)) for t in tuples])
    for t, o in zip(tuples, out):
        assert int(o) == memo_hash(t)
    for entries in (1024, 1 << 20, 1 << 32):
        out = run(prog, [f"bucket {entries} " + " ".join(map(str, t)) for t in tuples])
        for t, o in zip(tuples, out):
            b, tag = (int(x) for x in o.split())
            h = memo_hash(t)
            assert b == h & (entries - 1) and tag == tag_of(h) and tag not in (0, 1)


def test_hash_spreads(prog):
    """One bit changed in any of the 25 words moves the bucket: over 25 x 32
    single-bit neighbours of one tuple at 1,024 buckets, no bucket holds more
    than a handful (a uniform spread gives a maximum near 5), and the tag
    changes with the bucket left out."""
    rng = random.Random(13)
    base = [rng.randrange(1 << 32) for _ in range(TUPLE_WORDS)]
    near = []
    for w in range(TUPLE_WORDS):
        for bit in range(32):
            t = list(base)
            t[w] ^= 1 << bit
            near.append(t)
    out = run(prog, ["bucket 1024 " + " ".join(map(str, t)) for t in near])
    buckets = [int(o.split()[0]) for o in out]
    tags = {int(o.split()[1]) for o in out}
    assert max(buckets.count(b) for b in set(buckets)) <= 8
    assert len(set(buckets)) > 500 and len(tags) > 790


def test_probe_sequence(prog):
    P = probe_steps(prog)
    cases = [(1024, 0), (1024, 1023), (1024, 1020), (1 << 20, (1 << 64) - 1), (1 << 32, (1 << 63) + 5), (2048, 2047 - P + 1)]
    out = run(prog, [f"probe {e} {h}" for e, h in cases])
    for (e, h), o in zip(cases, out):
        seq = [int(x) for x in o.split()]
        assert seq == [(h + j) & (e - 1) for j in range(P)]  # the home bucket, then linear, wrapping
        assert len(set(seq)) == P


def rotation_model(entries, passes):
    thr = entries // 4 * 3
    young = calls = rot = 0
    res = []
    for c in passes:
        calls += c
        due = calls >= thr
        if due:
            young ^= 1
            calls = 0
            rot += 1
        res.append((int(due), young, rot))
    return res


def test_rotation_rule(prog):
    rng = random.Random(14)
    scripts = [(1024, [767, 1, 768, 100, 667, 1]), (1024, [0, 0, 768]), (1024, [5000, 5000]), (4096, [1] * 10)]
    scripts += [(1 << rng.randrange(10, 16), [rng.randrange(0, 3000) for _ in range(200)]) for _ in range(20)]
    out = run(prog, [f"rotate {e} " + " ".join(map(str, p)) for e, p in scripts])
    for (e, p), o in zip(scripts, out):
        v = [int(x) for x in o.split()]
        assert [tuple(v[i:i + 3]) for i in range(0, len(v), 3)] == rotation_model(e, p)
    # 3/4 of a generation: 767 calls do not rotate 1,024 entries, the 768th does
    assert rotation_model(1024, [767, 1])[0][0] == 0 and rotation_model(1024, [767, 1])[1] == (1, 1, 1)


def test_scratch_sizes(prog):
    ns = [1, 63, 64, 65, 1000, 4096, 70000, 3 * (1 << 20)]
    out = run(prog, [f"scratch {n}" for n in ns])
    al = lambda x: (x + 63) & ~63  # noqa: E731
    for n, o in zip(ns, out):
        cnt, e, r, s, slot, origin, status, total = (int(x) for x in o.split())
        assert cnt == 0 and e == 64  # the miss counter in a 64-byte block of its own
        assert r - e >= 32 * n and s - r >= 32 * n and slot - s >= 32 * n
        assert origin - slot >= 4 * n and status - origin >= 4 * n and total - status >= n
        assert all(x % 64 == 0 for x in (e, r, s, slot, origin, status, total))
        assert total == 64 + 3 * al(32 * n) + 2 * al(4 * n) + al(n)


def test_verify_plan_memo_flag(prog):
    """verify_plan itself never sets memo; verify_plan_memo sets it, and a
    memo pass's plan does not account (the pass does, over its original items)."""
    cases = [(n, hc, acc, memo) for n in (1, 300, 4096, 5000, 70000) for hc in (0, 1) for acc in (0, 1) for memo in (0, 1)]
    out = run(prog, [f"plan {n} {hc} {acc} {memo}" for n, hc, acc, memo in cases])
    forms = {}
    for (n, hc, acc, memo), o in zip(cases, out):
        form, p_acc, p_memo, base_memo = (int(x) for x in o.split())
        assert base_memo == 0 and p_memo == memo
        assert p_acc == (acc if not memo else 0)
        forms.setdefault((n, hc), set()).add(form)
    assert all(len(f) == 1 for f in forms.values())  # the flags never change the form


def test_memo_plan_under_sanitizers(prog, tmp_path):
    """The same stand-alone program built with AddressSanitizer and UBSan and
    run as a program over every command."""
    exe = str(tmp_path / "memo_plan_check_san")
    # (host code only: the sanitizers are named for the host side of the compile and no GPU code is built)
    p = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-x", "c++", "-Xarch_host", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, SRC], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    t = list(range(1, 26))
    out = run(exe, ["geometry 262144", "geometry 1099511627776", "consts", "hash " + " ".join(map(str, t)),
                    "bucket 1024 " + " ".join(map(str, t)), "probe 1024 1023", "rotate 1024 767 1 768",
                    "scratch 70000", "plan 5000 0 1 1", "bucket 1000 1", "nonsense"])
    assert out[0] == "1024 262144" and out[1] == f"{1 << 32} {1 << 40}"
    assert int(out[3]) == memo_hash(t)
    assert out[4] == f"{memo_hash(t) & 1023} {tag_of(memo_hash(t))}"
    assert out[6] == "0 0 0 1 1 1 1 0 2"
    assert out[-2:] == ["error", "error"]
