"""The signed compact key class's recoding (minbft_amd/csrc/teeth_dev.h:
steeth_flip, teeth_pick) compiled for the HOST into the stand-alone program
tests/steeth_check (tests/csrc/steeth_check.cpp) and checked against Python
integers for every t in 2..9 over 10,000 random scalars in [1, N) and the
corners (1, 2, 3, N - 1, N - 2, N - 3, 2^255, 2^255 + 1, single bits on both
sides of every tooth boundary, all-same-sign columns, the ragged top, the
derived degenerate scalars):

* the flip (an even u is evaluated as N - u);
* each column's table index and sign, against the digits' definition;
* the columns rebuild k;
* every prefix of the evaluation lies in (0, N);
* the integer model meets a degenerate addition only at the last column of
  the scalars derived from k == 2 val_0(k) (mod N), and does meet it there.

The unsigned class goes through the same column picker now: its columns are
checked against tests/teeth_util.py too.  The program is also built with
AddressSanitizer and UBSan and run as a program (host code only).  The GPU
run is compared with the oracle in tests/test_gpu_signed_compact_keys.py."""
import os
import random
import subprocess

import pytest

import teeth_util
from steeth_util import (N, STEETH, column_list, columns, corner_scalars, degenerate_scalars, entry_mult, flip,
                         model)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "tests", "csrc", "steeth_check.cpp")


@pytest.fixture(scope="module")
def prog():
    from __graft_entry__ import build_steeth_check
    return build_steeth_check()


def run(exe, lines):
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    out = p.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def scalars_of(t, count):
    rng = random.Random(0x51ee7 + t)
    return [rng.randrange(1, N) for _ in range(count)] + corner_scalars(t)


def check_recoding(exe, t, count):
    us = scalars_of(t, count)
    d = columns(t)
    assert run(exe, ["cols %d" % t]) == [str(d)]
    degen_k = set(degenerate_scalars(t))
    seen = set()
    for u, line in zip(us, run(exe, ["rec %d %064x" % (t, u) for u in us])):
        f = line.split()
        k, flipped = flip(u)
        assert (int(f[0]), int(f[1], 16)) == (int(flipped), k), hex(u)
        cols = [(int(x) >> 1, bool(int(x) & 1)) for x in f[2:]]
        assert len(cols) == d and cols == column_list(k, t), hex(u)
        assert cols[0][1] is False                       # the top column is positive
        assert all(idx < 1 << (t - 1) for idx, _ in cols)
        m, outside, degen = model(cols, t)
        assert m == k, hex(u)                            # the columns rebuild k
        assert not outside, (hex(u), outside[:2])        # every prefix in (0, N)
        if k in degen_k:
            assert [s for s, _, _ in degen] == [d - 1], (hex(u), degen)
            seen.add(u)
        else:
            assert not degen, (hex(u), degen[:2])
    # both scalars of every derived pair were run (the odd k and the even N - k)
    assert seen == degen_k | {N - k for k in degen_k}


@pytest.mark.parametrize("t", list(STEETH))
def test_recoding_against_python_integers(prog, t):
    check_recoding(prog, t, 10000)


def test_derived_degenerate_scalars():
    """Two scalars each for t = 2, 3, 8, 9, none for t = 4..7; each is where
    the condition says."""
    for t in STEETH:
        ks = degenerate_scalars(t)
        assert len(ks) == (1 if t in (2, 3, 8, 9) else 0), (t, ks)
        for k in ks:
            cols = column_list(k, t)
            idx, neg = cols[-1]
            v0 = -entry_mult(idx, t) if neg else entry_mult(idx, t)
            assert k & 1 and 0 < k < N and (k - 2 * v0) % N == 0
            assert not (N - k) & 1


@pytest.mark.parametrize("t", list(STEETH))
def test_table_multipliers(t):
    mult = [entry_mult(i, t) for i in range(1 << (t - 1))]
    assert all(m & 1 and 0 < m < 1 << 234 for m in mult)  # (t - 1) d <= 232, at t = 9
    assert len(set(mult)) == len(mult)


def test_refused_teeth(prog):
    u = "%064x" % 5
    assert run(prog, ["cols 1", "cols 10", "cols 0", "cols -1", "rec 1 " + u, "rec 10 " + u, "urec 9 " + u]) == ["-1"] * 7


@pytest.mark.parametrize("t", list(teeth_util.TEETH))
def test_unsigned_columns_through_the_shared_picker(prog, t):
    rng = random.Random(0x7ee7 + t)
    us = [rng.randrange(1, 1 << 256) for _ in range(1000)] + teeth_util.corner_scalars(t)
    for u, line in zip(us, run(prog, ["urec %d %064x" % (t, u) for u in us])):
        want = [v if v else -1 for v in teeth_util.column_values(u, t)]
        assert [int(x) for x in line.split()] == want, hex(u)


def test_recoding_under_sanitizers(tmp_path):
    """The same stand-alone program built with AddressSanitizer and UBSan and
    run as a program, every t over 300 random scalars and the corners."""
    exe = str(tmp_path / "steeth_check_san")
    # (host code only: the sanitizers are named for the host side of the compile and no GPU code is built)
    p = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, SRC], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    for t in STEETH:
        check_recoding(exe, t, 300)
