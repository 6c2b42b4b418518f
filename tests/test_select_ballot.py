"""The ballot select's formulation (csrc/mz_tree_device.h select_path_ballot)
against a serial walk, on the CPU.

A tree of at most 64 expanded nodes (slot 0 = the root, a child's slot is
larger than its parent's) carries per node the statics par / dep / act and
the ancestor mask anc[n] = anc[par[n]] | 1 << n, and a cache entry that is
either current (it names the action select takes there and the child slot
that edge leads to, or none) or not (stale, tied, never computed).

The serial walk follows current entries from the root until it reaches an
unexpanded edge (the leaf) or a node whose entry is not current (where the
full evaluation takes over).  The ballot form decides the same thing with
one vote per node: ok[n] = "n's parent is current and chooses n", OK =
ballot(ok) | 1, n is on the path iff anc[n] is a subset of OK, the path's
end is the highest on-path slot and its depth is popcount - 1.  Leaf, stop
node and every path entry must be identical.
"""
import numpy as np
import pytest

SENTINEL = -7          # path entries neither form may touch


def _random_tree(rng, n_nodes, A, p_stale, chain=False):
    """par/dep/act per node, child[n][a] = slot or -1, and the cache:
    cur[n], cact[n] (chosen action), cch[n] (chosen child slot + 1, 0 = none)."""
    par = np.zeros(n_nodes, np.int64)
    dep = np.zeros(n_nodes, np.int64)
    act = np.zeros(n_nodes, np.int64)
    child = -np.ones((n_nodes, A), np.int64)
    for n in range(1, n_nodes):
        for _ in range(1000):
            p = n - 1 if chain else int(rng.integers(0, n))
            free = np.flatnonzero(child[p] < 0)
            if len(free):
                break
        a = int(rng.choice(free))
        par[n], dep[n], act[n] = p, dep[p] + 1, a
        child[p, a] = n
    anc = [1] * n_nodes
    for n in range(1, n_nodes):
        anc[n] = anc[par[n]] | (1 << n)
    cur = rng.random(n_nodes) >= p_stale
    cact = rng.integers(0, A, n_nodes)
    cch = np.array([child[n, cact[n]] + 1 for n in range(n_nodes)], np.int64)
    return par, dep, act, anc, cur, cact, cch


def _serial(par, dep, act, cur, cact, cch, A):
    """(found, node, leaf action, depth of `node`, path) by the level walk."""
    path = {}
    e, d = 0, 0
    while True:
        if not cur[e]:
            return False, e, -1, d, path
        a = int(cact[e])
        d += 1
        if cch[e] == 0:
            path[d] = (e * A + a, -1)
            return True, e, a, d - 1, path
        c = int(cch[e]) - 1
        path[d] = (e * A + a, c)
        e = c


def _ballot(par, dep, act, anc, cur, cact, cch, A):
    n_nodes = len(par)
    OK = 1
    for n in range(1, n_nodes):
        if cur[par[n]] and cch[par[n]] - 1 == n:
            OK |= 1 << n
    ON = 0
    path = {}
    for n in range(n_nodes):
        if anc[n] & ~OK == 0:
            ON |= 1 << n
            if n >= 1:
                path[int(dep[n])] = (int(par[n]) * A + int(act[n]), n)
    L = ON.bit_length() - 1
    D = bin(ON).count("1") - 1
    assert D == dep[L], "the highest on-path slot is not the deepest"
    if cur[L]:
        assert cch[L] == 0, "a current chain end must choose an unexpanded edge"
        a = int(cact[L])
        path[D + 1] = (L * A + a, -1)
        return True, L, a, D, path
    return False, L, -1, D, path


def _check(tree, A):
    par, dep, act, anc, cur, cact, cch = tree
    s = _serial(par, dep, act, cur, cact, cch, A)
    b = _ballot(par, dep, act, anc, cur, cact, cch, A)
    assert s[:4] == b[:4], f"serial {s[:4]} != ballot {b[:4]}"
    assert s[4] == b[4], "path entries differ"


@pytest.mark.parametrize("p_stale", [0.0, 0.1, 0.5, 1.0])
def test_random_trees(p_stale):
    rng = np.random.default_rng(int(p_stale * 100) + 1)
    for _ in range(500):
        n_nodes = int(rng.integers(1, 65))
        A = int(rng.integers(2, 10))
        _check(_random_tree(rng, n_nodes, A, p_stale), A)


def test_single_node():
    rng = np.random.default_rng(5)
    for p_stale in (0.0, 1.0):
        _check(_random_tree(rng, 1, 9, p_stale), 9)


@pytest.mark.parametrize("n_nodes", [2, 17, 64])
def test_chain(n_nodes):
    """one child per node: the path reaches depth n_nodes - 1 (past the 16
    register-held levels of the serial walk), slot 63 and mask bit 63 at 64."""
    rng = np.random.default_rng(n_nodes)
    for p_stale in (0.0, 0.05, 0.3):
        for _ in range(200):
            _check(_random_tree(rng, n_nodes, 3, p_stale, chain=True), 3)
    tree = _random_tree(rng, n_nodes, 3, 0.0, chain=True)
    par, dep, act, anc, cur, cact, cch = tree
    for n in range(n_nodes - 1):                    # every entry follows the chain
        cact[n], cch[n] = act[n + 1], n + 2
    _check(tree, 3)
    found, node, _, D, path = _ballot(*tree, 3)
    assert found and node == n_nodes - 1 and D == n_nodes - 1 and len(path) == n_nodes
