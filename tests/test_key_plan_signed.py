"""The signed compact class in the key store's bookkeeping
(minbft_amd/csrc/key_plan.h), through the stand-alone program
tests/key_plan_check: the bytes of the codes 0x202 .. 0x209, the codes next to
them refused, and promotion order across unsigned, signed and window classes,
the byte ties (signed t against unsigned t - 1) included."""
import subprocess

import pytest


def S(t):
    return 0x200 | t


def T(t):
    return 0x100 | t


@pytest.fixture(scope="module")
def prog():
    from __graft_entry__ import build_key_plan_check
    return build_key_plan_check()


def run(exe, lines):
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return p.stdout.splitlines()


def test_bytes_of_signed_classes(prog):
    out = run(prog, ["bytes %d" % S(t) for t in range(2, 10)])
    assert [int(x) for x in out] == [64 << (t - 1) for t in range(2, 10)]
    assert [int(x) for x in out] == [128, 256, 512, 1024, 2048, 4096, 8192, 16384]


def test_neighbouring_codes_are_unknown(prog):
    codes = [0x200, 0x201, 0x20A, 0x20B, 0x2FF, 0x300, 0x302, 0x100, 0x101, 0x109]
    assert run(prog, ["bytes %d" % c for c in codes]) == ["-1"] * len(codes)
    # the unsigned class reads as before
    assert [int(x) for x in run(prog, ["bytes %d" % T(t) for t in range(2, 9)])] == [64 << t for t in range(2, 9)]


def test_signed_pieces_are_listed_by_class(prog):
    """A released signed piece is reused by its own class only, not by the
    unsigned class of the same bytes."""
    out = run(prog, ["reg 1 %d" % S(5), "reg 2 %d" % T(4), "rem 1", "reg 3 %d" % T(4), "reg 4 %d" % S(5), "rem 2",
                     "reg 5 %d" % S(5), "reg 6 %d" % T(4)])
    p1, p2, _, p3, p4, _, p5, p6 = (int(x) for x in out)
    assert p2 - p1 == 1024 and p3 not in (p1, p2) and p4 == p1 and p5 not in (p1, p2, p3) and p6 == p2


def promote(prog, rows, cls, max_keys, min_uses):
    lines = ["promote %d %d %d %d" % (len(rows), cls, max_keys, min_uses)]
    lines += ["%d %d %d" % row for row in rows]
    return [int(x) for x in run(prog, lines)[0].split()]


def test_promotion_order_across_classes(prog):
    # (uses, class, valid)
    rows = [(50, 0, 1),       # 0: 64 B
            (90, S(2), 1),    # 1: 128 B
            (80, T(2), 1),    # 2: 256 B
            (70, S(3), 1),    # 3: 256 B
            (95, T(4), 1),    # 4: 1 KiB -- ties with signed 5
            (99, S(5), 1),    # 5: 1 KiB
            (60, S(6), 1),    # 6: 2 KiB
            (85, 4, 1),       # 7: 32 KiB
            (88, S(4), 0),    # 8: invalid
            (75, S(9), 1)]    # 9: 16 KiB
    # into signed 5 (1 KiB): the cheaper classes by uses; neither the tie nor itself
    assert promote(prog, rows, S(5), 10, 0) == [1, 2, 3, 0]
    # into unsigned 4 (1 KiB): the same keys -- signed 5 is not promoted into it
    assert promote(prog, rows, T(4), 10, 0) == [1, 2, 3, 0]
    # into signed 3 (256 B): unsigned 2 ties and stays
    assert promote(prog, rows, S(3), 10, 0) == [1, 0]
    assert promote(prog, rows, T(2), 10, 0) == [1, 0]
    # into W = 4: everything valid below 32 KiB, most used first; max_keys and min_uses cut
    assert promote(prog, rows, 4, 10, 0) == [5, 4, 1, 2, 9, 3, 6, 0]
    assert promote(prog, rows, 4, 3, 0) == [5, 4, 1]
    assert promote(prog, rows, 4, 10, 80) == [5, 4, 1, 2]
    # into signed 9 (16 KiB): unsigned 8 would tie; signed 6 and below move
    assert promote(prog, rows + [(100, T(8), 1)], S(9), 10, 0) == [5, 4, 1, 2, 3, 6, 0]
    # into signed 2 (128 B): only the table-free key
    assert promote(prog, rows, S(2), 10, 0) == [0]
