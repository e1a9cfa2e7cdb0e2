"""Greedy all-pairs covering arrays over named factors with named constraints (no third-party dependency beyond numpy).

    factors     = {"taps": [1, 9], "wrap": [False, True], ...}               # ordered
    constraints = [("taps1_no_wrap", lambda c: c["taps"] == 9 or not c["wrap"], "kernels.py:598: 1x1 has no columns to wrap"), ...]
    cases       = cover(factors, legal_from(constraints), seeds, rng_seed=0)

``cover`` enumerates the legal part of the full product (the tables here have at most a few tens of thousands of assignments),
puts the seeds first and then repeatedly adds the legal assignment that covers the most value pairs not covered yet, until every
pair that occurs in SOME legal assignment occurs in a case.  Deterministic: ties go to the first candidate in an order shuffled
once by ``numpy.random.RandomState(rng_seed)`` (the legacy generator, whose streams are frozen).
"""
import itertools

import numpy as np


def legal_from(constraints):
    """(name, predicate, reason) triples -> legal(case); ``why(case)`` on the result names the constraints a case breaks."""
    names = [n for n, _, _ in constraints]
    assert len(set(names)) == len(names), "constraint names must be unique"
    for n, p, reason in constraints:
        assert callable(p) and isinstance(reason, str) and reason, n

    def legal(case):
        return all(p(case) for _, p, _ in constraints)

    legal.why = lambda case: [n for n, p, _ in constraints if not p(case)]
    legal.constraints = constraints
    return legal


def _enumerate(factors, legal):
    names = list(factors)
    rows = [idx for idx in itertools.product(*(range(len(factors[n])) for n in names))
            if legal({n: factors[n][i] for n, i in zip(names, idx)})]
    return names, np.asarray(rows, dtype=np.int64).reshape(len(rows), len(names))


def _index(factors, case):
    return [factors[n].index(case[n]) for n in factors]


def _pairs_of(rows, sizes):
    """bool [F, F, Vmax, Vmax]: entry (i, j, a, b), i < j, is set when some row has value a of factor i and b of factor j."""
    nf, vmax = len(sizes), max(sizes)
    seen = np.zeros((nf, nf, vmax, vmax), dtype=bool)
    for i in range(nf):
        for j in range(i + 1, nf):
            seen[i, j, rows[:, i], rows[:, j]] = True
    return seen


def cover(factors, legal, seeds=(), rng_seed=0, cost=None):
    """List of dicts {factor: value}: the seeds (each must be legal; keys outside ``factors``, such as "site", are kept), then greedy
    picks until every legal pair is covered.  ``cost(case)``: among candidates that cover equally many new pairs the cheapest wins
    (the expensive launch classes then appear only where a pair needs them)."""
    names, rows = _enumerate(factors, legal)
    assert len(rows), "no legal assignment"
    sizes = [len(factors[n]) for n in names]
    todo = _pairs_of(rows, sizes)
    cases = []
    for s in seeds:
        core = {n: s[n] for n in names}
        assert legal(core), ("illegal seed", s, getattr(legal, "why", lambda c: "?")(core))
        idx = np.asarray([_index(factors, core)])
        todo &= ~_pairs_of(idx, sizes)
        cases.append(dict(s))
    rows = rows[np.random.RandomState(rng_seed).permutation(len(rows))]
    if cost is not None:
        price = np.asarray([cost({n: factors[n][int(v)] for n, v in zip(names, r)}) for r in rows])
        rows = rows[np.argsort(price, kind="stable")]
    nf = len(names)
    while todo.any():
        score = np.zeros(len(rows), dtype=np.int64)
        for i in range(nf):
            for j in range(i + 1, nf):
                score += todo[i, j, rows[:, i], rows[:, j]]
        best = int(score.argmax())
        assert score[best] > 0
        pick = rows[best:best + 1]
        todo &= ~_pairs_of(pick, sizes)
        cases.append({n: factors[n][int(v)] for n, v in zip(names, pick[0])})
    return cases


def legal_pairs(factors, legal):
    """Set of ((factor i, value), (factor j, value)), i before j, that occur in some legal assignment."""
    names, rows = _enumerate(factors, legal)
    seen = _pairs_of(rows, [len(factors[n]) for n in names]) if len(rows) else np.zeros((0, 0, 0, 0), dtype=bool)
    return {((names[i], factors[names[i]][a]), (names[j], factors[names[j]][b])) for i, j, a, b in zip(*np.nonzero(seen))}


def uncovered(cases, factors, legal):
    """The pairs that occur in some legal assignment and in no case (sorted list; empty when the cases cover the table)."""
    names = list(factors)
    have = set()
    for c in cases:
        for i in range(len(names)):
            for j in range(i + 1, len(names)):
                have.add(((names[i], c[names[i]]), (names[j], c[names[j]])))
    return sorted(legal_pairs(factors, legal) - have, key=repr)
