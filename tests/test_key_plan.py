"""The key store's bookkeeping after registration (minbft_amd/csrc/key_plan.h):
released slot numbers, per-class lists of released storage pieces, the dirty
ranges of the descriptor upload and the promotion choice, plus the use-count
stage's part of the launch plan (verify_plan.h) -- all plain C++, driven
through the stand-alone program tests/key_plan_check (built by
__graft_entry__.build() from tests/csrc/key_plan_check.cpp) and compared with
models written here.  No GPU."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "key_plan_check.cpp")
HIPCC = "/opt/rocm/bin/hipcc"

TEETH = 0x100
CLASSES = [0] + [TEETH | t for t in range(2, 9)] + list(range(4, 30))


def class_bytes(cls):
    """Bytes of one key's data, restated from the class definitions: 64 B an
    entry; one entry (table-free), 2^t (compact), the signed comb's
    (S - 1) 2^(W-1) + 2^(256 - (S-1) W) with S = ceil(256 / W)."""
    if cls == 0:
        return 64
    if cls >= TEETH:
        return 64 << (cls & 0xFF)
    s = -(-256 // cls)
    return 64 * (((s - 1) << (cls - 1)) + (1 << (256 - (s - 1) * cls)))


@pytest.fixture(scope="module")
def prog():
    import __graft_entry__ as ge
    return ge.build_key_plan_check()


def run(prog, lines):
    p = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return p.stdout.split("\n")[:-1]


def test_class_bytes_and_codes(prog):
    codes = list(range(0, 40)) + list(range(TEETH, TEETH + 12)) + [0x200, 0xFFFFFFFF]
    out = run(prog, [f"bytes {c}" for c in codes])
    for c, o in zip(codes, out):
        assert int(o) == (class_bytes(c) if c in CLASSES else -1), c
    # the documented sizes: 520 entries at W = 4 (63 windows of 8, one of 16), 1 KiB at t = 4, 16 KiB at t = 8
    assert class_bytes(4) == 520 * 64 and class_bytes(TEETH | 4) == 1 << 10 and class_bytes(TEETH | 8) == 16 << 10


def test_slot_reuse_lowest_first(prog):
    rng = random.Random(5)
    free, cmds, want = set(), [], []
    for _ in range(3000):
        if rng.random() < 0.55:
            s = rng.randrange(500)
            free.add(s)
            cmds.append(f"srel {s}")
            want.append(len(free))
        else:
            cmds.append("stake")
            if free:
                s = min(free)
                free.remove(s)
                want.append(s)
            else:
                want.append(-1)
    assert [int(x) for x in run(prog, cmds)] == want
    # the lowest numbers a many-key registration will take, looked at without taking them
    out = run(prog, ["srel 9", "srel 3", "srel 7", "slow 2", "slow 0", "slow 10", "stake", "slow 10"])
    assert [o.split() for o in out[3:]] == [["3", "7"], [], ["3", "7", "9"], ["3"], ["7", "9"]]


def piece_model_ops(seed, nops):
    """10,000 random register / remove / re-class operations and what a
    model of the piece lists answers: a piece is taken from its class's list
    (last released first) or made fresh by a bump allocator from 0x1000."""
    rng = random.Random(seed)
    classes = [0, TEETH | 2, TEETH | 4, TEETH | 8, 4, 8]
    lists = {c: [] for c in classes}
    keys, live, nxt, fresh = {}, set(), 0x1000, 0
    made = set()
    cmds, want = [], []

    def piece_for(cls):
        nonlocal nxt, fresh
        if lists[cls]:
            p = lists[cls].pop()
        else:
            p = nxt
            nxt += class_bytes(cls)
            fresh += 1
            made.add((cls, p))
        assert p not in live, "piece handed out twice"
        live.add(p)
        return p

    for k in range(nops):
        r = rng.random()
        if not keys or r < 0.4:
            cls = rng.choice(classes)
            p = piece_for(cls)
            keys[k] = (cls, p)
            cmds.append(f"reg {k} {cls}")
            want.append(p)
        elif r < 0.7:
            key = rng.choice(list(keys))
            cls, p = keys.pop(key)
            live.remove(p)
            lists[cls].append(p)
            cmds.append(f"rem {key}")
            want.append(p)
        else:
            key = rng.choice(list(keys))
            cls = rng.choice(classes)
            p = piece_for(cls)  # the new piece first, then the old one goes back
            ocls, op = keys[key]
            live.remove(op)
            lists[ocls].append(op)
            keys[key] = (cls, p)
            cmds.append(f"rec {key} {cls}")
            want.append(p)
        if k % 500 == 499:
            # none lost: every piece ever made is held by a key or on its list
            listed = {(c, p) for c in classes for p in lists[c]}
            held = {(c, p) for c, p in keys.values()}
            assert listed | held == made and not (listed & held)
            cmds.append("pstat")
            want.append((sum(len(v) for v in lists.values()),
                         sum(class_bytes(c) * len(v) for c, v in lists.items()), fresh, len(live)))
    return cmds, want


def check_pieces(prog):
    cmds, want = piece_model_ops(17, 10000)
    out = run(prog, cmds)
    assert len(out) == len(want)
    for c, o, w in zip(cmds, out, want):
        got = tuple(int(x) for x in o.split()) if c == "pstat" else int(o)
        assert got == w, (c, got, w)


def test_piece_lists_against_model(prog):
    check_pieces(prog)


def dirty_model(marks):
    cover = set()
    for lo, hi in marks:
        cover.update(range(lo, hi))
    out, run_lo, prev = [], None, None
    for i in sorted(cover):
        if run_lo is None:
            run_lo = i
        elif i != prev + 1:
            out.append((run_lo, prev + 1))
            run_lo = i
        prev = i
    if run_lo is not None:
        out.append((run_lo, prev + 1))
    return out


def test_dirty_ranges_coalesce(prog):
    rng = random.Random(23)
    cases = [[(5, 6)], [(5, 6), (6, 7)], [(6, 7), (5, 6)], [(0, 3), (10, 12), (3, 10)], [(4, 9), (1, 20)],
             [(1, 20), (4, 9)], [(7, 7)], [(2, 4), (6, 8), (4, 6)], [(999999, 1000000)]]
    for _ in range(200):
        cases.append([(lo, lo + rng.randrange(0, 6)) for lo in (rng.randrange(120) for _ in range(rng.randrange(1, 30)))])
    cmds = []
    for marks in cases:
        cmds += [f"mark {lo} {hi}" for lo, hi in marks] + ["dirty"]
    out = [o for o in run(prog, cmds) if o != "ok"]
    assert len(out) == len(cases)
    for marks, o in zip(cases, out):
        got = [tuple(int(x) for x in r.split("-")) for r in o.split()]
        assert got == dirty_model(marks), marks
    # one key among a million slots: one entry (16 B) goes up, not the array
    assert dirty_model([(123456, 123457)]) == [(123456, 123457)]


def promotion_model(rows, cls, max_keys, min_uses):
    """valid keys of a class cheaper in memory than cls with uses >= min_uses;
    the max_keys most used, ties to the lower slot."""
    cand = [i for i, (u, c, v) in enumerate(rows) if v and u >= min_uses and class_bytes(c) < class_bytes(cls)]
    cand.sort(key=lambda i: (-rows[i][0], i))
    return cand[:max_keys]


def test_promotion_choice(prog):
    rng = random.Random(31)
    cases = []
    # ties, keys at or above the target left alone, invalid keys, the 0-uses floor
    cases.append(([(10, 0, 1), (10, 0, 1), (11, 0, 1), (10, 8, 1), (50, 16, 1), (99, 0, 0), (3, TEETH | 4, 1)], 8, 3, 5))
    cases.append(([(0, 0, 1)] * 4, TEETH | 2, 10, 0))
    cases.append(([(5, 0, 1)] * 4, 0, 10, 0))           # nothing is cheaper than table-free
    cases.append(([(5, TEETH | 8, 1), (5, 4, 1)], 4, 10, 0))  # t = 8 (16 KiB) is cheaper than W = 4 (32 KiB)
    for _ in range(150):
        n = rng.randrange(1, 80)
        rows = [(rng.choice([0, 1, 2, 5, 5, 100, rng.randrange(1 << 40)]), rng.choice(CLASSES), int(rng.random() < 0.9))
                for _ in range(n)]
        cases.append((rows, rng.choice(CLASSES), rng.choice([0, 1, 2, 5, n, 2 * n]), rng.choice([0, 1, 5, 6, 101])))
    cmds = []
    for rows, cls, mk, mu in cases:
        cmds.append(f"promote {len(rows)} {cls} {mk} {mu}")
        cmds += [f"{u} {c} {v}" for u, c, v in rows]
    out = run(prog, cmds)
    assert len(out) == len(cases)
    for (rows, cls, mk, mu), o in zip(cases, out):
        assert [int(x) for x in o.split()] == promotion_model(rows, cls, mk, mu), (rows, cls, mk, mu)


def test_account_stage_in_the_plan(prog):
    """The stage is off unless asked for, changes nothing else of the plan, and
    its grid is one block per 256 items up to 4 blocks per CU."""
    out = run(prog, ["plan 100000 0", "plan 100000 1", "blocks 1 256", "blocks 256 256", "blocks 257 256",
                     "blocks 66000 256", "blocks 1048576 256", "blocks 1048576 8"])
    assert out[0] == "0 0 1 100000" and out[1] == "0 1 1 100000"
    assert [int(x) for x in out[2:]] == [1, 1, 2, 258, 1024, 32]


def test_key_plan_under_sanitizers(prog, tmp_path):
    """The same stand-alone program built with AddressSanitizer and UBSan and
    run as a program over the piece-list and range operations."""
    exe = str(tmp_path / "key_plan_check_san")
    # (host code only: the sanitizers are named for the host side of the compile and no GPU code is built)
    p = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-x", "c++", "-Xarch_host", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, SRC], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    check_pieces(exe)
    out = run(exe, ["mark 3 9", "mark 1 4", "mark 20 21", "dirty", "srel 4", "srel 2", "stake", "stake", "stake"])
    assert out[3].split() == ["1-9", "20-21"] and out[-3:] == ["2", "4", "-1"]
