"""Shared cases of the network-only player's tests: fixed policy
rows p with their legal masks, the draws and temperatures every row is played
at, the oracle's det_exp / det_log as prior_pick's detmath, and the text form
the sanitizer harness (tests/sanitize/prior_rules_main.cpp) reads and writes.
"""
import struct

import numpy as np

DRAWS = (0, 0x55555556, 0xFFFFFFFF)
TEMPS = (0.0, 1.0, float("inf"), 0.5, 4.0)


class OracleMath:
    """det_exp / det_log of include/mz_detmath.h through the CPU oracle."""

    def __init__(self):
        import oracle
        self.L = oracle.lib()

    def det_exp(self, x):
        return self.L.ora_det_exp(float(x))

    def det_log(self, x):
        return self.L.ora_det_log(float(x))


def _softmax32(x):
    e = np.exp((x - x.max()).astype(np.float64))
    return (e / e.sum()).astype(np.float32)


def rows():
    """[(name, p (A,) float32, legal (A,) bool)] for A = 9 and A = 7."""
    out = []
    for A in (9, 7):
        rng = np.random.default_rng(100 + A)
        p = _softmax32(rng.normal(0, 2, A))
        full = np.ones(A, bool)
        out.append((f"A{A}-all-legal", p, full))
        for k in (0, A // 2, A - 1):
            one = np.zeros(A, bool)
            one[k] = True
            out.append((f"A{A}-one-legal-{k}", p, one))
        for j in range(4):
            m = rng.random(A) < 0.5
            m[rng.integers(A)] = True
            out.append((f"A{A}-random-{j}", _softmax32(rng.normal(0, 3, A)), m))
        # every legal entry is 0 (the policy's mass sits on illegal actions): the uniform fallback
        m = np.zeros(A, bool)
        m[[1, 3, A - 2]] = True
        z = p.copy()
        z[m] = 0.0
        out.append((f"A{A}-legal-all-zero", z, m))
        # two equal maxima among the legal actions (a larger illegal one in between): the first wins
        t = np.full(A, 0.05, np.float32)
        t[2] = t[5] = 0.25
        t[3] = 0.3
        m = np.ones(A, bool)
        m[3] = False
        out.append((f"A{A}-two-maxima", t, m))
        # a subnormal and a zero among the legal entries
        u = _softmax32(rng.normal(0, 1, A))
        u[0] = np.float32(1e-42)
        u[1] = 0.0
        out.append((f"A{A}-subnormal", u, full))
    return out


def cases():
    """Every row at every (temperature, draw): [(name, p, legal, T, r)]."""
    return [(n, p, m, T, r) for n, p, m in rows() for T in TEMPS for r in DRAWS]


def bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def case_line(p, legal, T, r):
    """One input line of the harness: A, the temperature's bits, r, the mask, p's bits (hex)."""
    return " ".join([str(len(p)), f"{bits(T):08x}", str(int(r)), "".join(str(int(b)) for b in legal)] +
                    [f"{bits(x):08x}" for x in p])


def result_line(action, pi):
    """What the harness prints for a row: the 0-based action and π's bits."""
    return " ".join([str(int(action))] + [f"{bits(x):08x}" for x in pi])
