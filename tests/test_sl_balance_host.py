"""The placement core of the sorted report lists (vimure_amd/csrc/sl_balance.h) on the host: invariants, determinism and the
modelled LDS cycles of a round, restated here in NumPy.

The model ("Planned placement"): a 16-byte read of row ym is served in four groups of 16 lanes --
{0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the two shifted by 32 -- on bank slot ym mod 16; lanes on one row share a cycle,
every further row on a slot costs one.  The 8-byte add is served in four contiguous groups of 16 lanes, slot ym mod 16, one cycle
per lane on a slot.  A round costs the sum over its groups of the fullest slot; empty entries cost nothing."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "sl_balance_host.cpp")
INC = os.path.join(ROOT, "vimure_amd", "csrc")

LANE = np.arange(64)
_q = LANE & 31
READ_GROUP = 2 * (LANE >> 5) + (((_q >= 4) & (_q < 12)) | ((_q >= 16) & (_q < 20)) | (_q >= 28)).astype(int)
ADD_GROUP = LANE >> 4


def model_cycles(step):
    """(read, add) cycles of a step [R, 64] of entries under the model."""
    rd = ad = 0
    for e in step:
        ym = (e & 0xFFFFF).astype(np.int64)
        live = e != 0
        for g in range(4):
            rows = np.unique(ym[live & (READ_GROUP == g)])
            if rows.size:
                rd += int(np.bincount(rows % 16, minlength=16).max())
            lanes = ym[live & (ADD_GROUP == g)]
            if lanes.size:
                ad += int(np.bincount(lanes % 16, minlength=16).max())
    return rd, ad


def make_step(rs, R, n_rep, Mp, short=False, far=False, one_reporter=False, p_level1=0.3):
    """A step as k_sl_place leaves it: every lane's reports ascending by reporter, rotated by a random offset; with `far`, the
    reports of mirror count 1 moved to the front as k_far_first does (lead = their number)."""
    step = np.zeros((R, 64), np.uint32)
    lead = np.zeros(64, np.uint32)
    for lane in range(64):
        n = R if not short else int(rs.randint(0, R + 1))
        n = min(n, n_rep)
        m = np.sort(rs.choice(n_rep, size=n, replace=False))
        if one_reporter and n:
            m[:] = 0
            m = m[:1]
            n = 1
        m = np.roll(m, -int(rs.randint(0, max(n, 1))))
        y = (rs.rand(n) < p_level1).astype(np.int64)
        x = rs.randint(1, 6, size=n)
        e = ((x << 21) | (1 << 20) | (y * Mp + m)).astype(np.uint32)
        if far and n:
            isfar = y > 0
            order = np.concatenate([np.flatnonzero(isfar), np.flatnonzero(~isfar)])
            e = e[order]
            lead[lane] = int(isfar.sum())
        step[:n, lane] = e
    return step, lead


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("slb") / "sl_balance_host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", INC, SRC, "-o", exe], check=True)
    return exe


def balance(exe, steps):
    """steps: list of (step [R, 64], lead [64]) -> list of (first call's output, second call's output)."""
    buf = b"".join(np.uint32(s.shape[0]).tobytes() + l.astype(np.uint32).tobytes() + np.ascontiguousarray(s, np.uint32).tobytes()
                   for s, l in steps)
    out = subprocess.run([exe], input=buf, stdout=subprocess.PIPE, check=True).stdout
    flat = np.frombuffer(out, np.uint32)
    assert flat.size == 2 * sum(s.size for s, _ in steps)
    res, at = [], 0
    for s, _ in steps:
        a = flat[at:at + s.size].reshape(s.shape)
        b = flat[at + s.size:at + 2 * s.size].reshape(s.shape)
        res.append((a, b))
        at += 2 * s.size
    return res


def check_invariants(step, lead, out, Mp):
    R = step.shape[0]
    for lane in range(64):
        cin, cout = step[:, lane], out[:, lane]
        n = int(np.flatnonzero(cin)[-1]) + 1 if cin.any() else 0
        ld = int(lead[lane])
        assert not cout[n:].any(), "an entry moved behind the tie's last report"
        assert np.all(cout[:n] != 0), "an empty entry moved in front of a report"
        for w0 in range(0, R, 8):   # permuted inside the windows of 8 rounds and inside the two segments only
            for lo, hi in ((w0, min(ld, w0 + 8)), (max(ld, w0), min(n, w0 + 8))):
                if hi > lo:
                    assert np.array_equal(np.sort(cin[lo:hi]), np.sort(cout[lo:hi])), (lane, lo, hi)
        assert np.all((cout[:ld] & 0xFFFFF) >= Mp) or ld == 0


CASES = [(R, n_rep, Mp) for R in (1, 2, 3, 4, 8, 19) for n_rep, Mp in ((24, 64), (200, 256))]


@pytest.mark.parametrize("R,n_rep,Mp", CASES)
def test_invariants_determinism_never_worse(prog, R, n_rep, Mp):
    rs = np.random.RandomState(1000 * R + n_rep)
    steps = [make_step(rs, R, n_rep, Mp),
             make_step(rs, R, n_rep, Mp, short=True),
             make_step(rs, R, n_rep, Mp, far=True),
             make_step(rs, R, n_rep, Mp, short=True, far=True),
             make_step(rs, R, n_rep, Mp, one_reporter=True),
             (np.zeros((R, 64), np.uint32), np.zeros(64, np.uint32))]
    for (step, lead), (a, b) in zip(steps, balance(prog, steps)):
        assert np.array_equal(a, b), "two calls on the same input differ"
        check_invariants(step, lead, a, Mp)
        r0, a0 = model_cycles(step)
        r1, a1 = model_cycles(a)
        assert r1 <= r0 and a1 <= a0, (r0, a0, r1, a1)


@pytest.mark.parametrize("R,least", [(2, 0.10), (4, 0.20), (8, 0.20)])
def test_modelled_cycles_fall(prog, R, least):
    rs = np.random.RandomState(77 + R)
    steps = [make_step(rs, R, 200, 256) for _ in range(20)]
    outs = balance(prog, steps)
    before = np.array([model_cycles(s) for s, _ in steps], float) / R
    after = np.array([model_cycles(a) for a, _ in outs], float) / R
    gain = 1.0 - after.mean(0) / before.mean(0)
    print(f"R={R}: read {before[:, 0].mean():.2f} -> {after[:, 0].mean():.2f}, add {before[:, 1].mean():.2f} -> {after[:, 1].mean():.2f} "
          f"cycles per round; gain read {gain[0]:.3f}, add {gain[1]:.3f}")
    assert gain[0] >= least and gain[1] >= least, gain
