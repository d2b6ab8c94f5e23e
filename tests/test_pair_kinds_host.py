"""Which primitive records share a pair record of a small scene's LDS image (host/gpu_layout.cpp pair_layout, through
the binding): arranged by kind, a leaf's triangles are paired with triangles and its spheres with spheres. CPU only.
"""
import itertools

import numpy as np
import pytest

import nori_hip as nh
import scenegen
from pair_kind_helpers import leaf_table
from primary_mask_records import PRIM_SPHERE, device_records, is_sphere


def _records(kinds):
    """(n, 12) float32 records, kinds[k] true = a sphere: only the kind bit matters to the arrangement."""
    rec = np.zeros((len(kinds), 12), np.float32)
    rec[:, 0] = np.arange(len(kinds))
    for k, sph in enumerate(kinds):
        if sph:
            rec[k, 11:12] = np.array([PRIM_SPHERE | 8], np.int32).view(np.float32)  # (another flag bit beside it)
        else:
            rec[k, 11:12] = np.array([2 | 4], np.int32).view(np.float32)  # flag bits without the sphere bit
    return rec


def _check(rec, leaves):
    """The by-kind arrangement of `leaves` over `rec` against the properties it promises; returns leaf_pairs."""
    slots, lp = nh.pair_layout(rec, leaves, by_kind=True)
    n = len(rec)
    assert slots.shape == (n, 2) and lp.shape == (len(leaves), 3)
    seen = np.zeros(n, int)
    used = np.zeros(n, bool)
    for (start, count), (first, n_tri, n_sph) in zip(leaves, lp):
        assert first == start
        tri = [k for k in range(start, start + count) if not is_sphere(rec[k])]
        sph = [k for k in range(start, start + count) if is_sphere(rec[k])]
        assert n_tri == (len(tri) + 1) // 2 and n_sph == (len(sph) + 1) // 2
        assert n_tri + n_sph <= max(count, 0)
        # triangle pairs first, then sphere pairs; each kind in the reference's record order, two by two
        want = [(v[i], v[i + 1] if i + 1 < len(v) else -1) for v in (tri, sph) for i in range(0, len(v), 2)]
        got = [tuple(int(x) for x in slots[first + i]) for i in range(n_tri + n_sph)]
        assert got == want, (leaves, got, want)
        for i, (a, b) in enumerate(got):
            assert not used[first + i]
            used[first + i] = True
            sphere_pair = i >= n_tri
            assert is_sphere(rec[a]) == sphere_pair
            seen[a] += 1
            if b >= 0:
                assert is_sphere(rec[b]) == sphere_pair and b > a  # no pair mixes kinds; indices are the reference's
                seen[b] += 1
        # at most one single triangle and one single sphere, each the last pair of its kind
        singles = [i for i, (_, b) in enumerate(got) if b < 0]
        assert all(i in (n_tri - 1, n_tri + n_sph - 1) for i in singles)
    in_leaf = np.zeros(n, int)
    for start, count in leaves:
        in_leaf[start:start + count] += 1
    np.testing.assert_array_equal(seen, in_leaf)  # every record of a leaf exactly once, no other record
    assert (slots[~used] == -1).all()  # positions no leaf uses
    return lp


@pytest.mark.parametrize("n", range(0, 11))
def test_every_mix_of_kinds(n):
    """One leaf of n records, every mix of kinds (all-triangle and all-sphere among them), at an even and an odd start."""
    for kinds in itertools.product((False, True), repeat=n):
        for start in (0, 1, 3):
            rec = _records([False] * start + list(kinds) + [True])  # (records outside the leaf on both sides)
            _check(rec, [(start, n)])


def test_several_leaves():
    """Leaves of sizes 0-10 one after the other, so most start at an odd record, with kinds drawn at random."""
    rng = np.random.default_rng(5)
    for trial in range(200):
        sizes = rng.permutation(11)[: rng.integers(1, 8)]
        kinds = rng.random(int(sizes.sum())) < rng.choice([0.1, 0.5, 0.9])
        leaves, k = [], 0
        for s in sizes:
            leaves.append((k, int(s)))
            k += int(s)
        _check(_records(kinds), leaves)


def test_reference_arrangement():
    """by_kind off: position p holds records (p, p + 1), the last one alone; every leaf's counts are 0."""
    rec = _records([False, True, False, False, True])
    slots, lp = nh.pair_layout(rec, [(0, 3), (3, 2)], by_kind=False)
    assert slots.tolist() == [[0, 1], [1, 2], [2, 3], [3, 4], [4, -1]]
    assert lp.tolist() == [[0, 0, 0], [3, 0, 0]]


def test_invalid_leaves_are_refused():
    rec = _records([False] * 4)
    for leaves in ([(0, 5)], [(-1, 2)], [(0, 3), (2, 2)], [(3, -1)]):
        with pytest.raises(nh.NoriError):
            nh.pair_layout(rec, leaves)


@pytest.mark.parametrize("variant", ["c1", "c2"])
def test_cornell_box(tmp_path, variant):
    """The Cornell box (the same tree for every variant): 4 triangle pairs + 1 sphere pair in leaf 0 -- the spheres are
    records 5 and 9 --, 2 triangle pairs in leaf 1."""
    s = nh.Scene(scenegen.cbox_xml(str(tmp_path), variant))
    b = nh.Bvh(s)
    rec, leaves = device_records(s, b), leaf_table(b)
    assert len(rec) == 14 and leaves == [(0, 10), (10, 4)]
    assert [k for k in range(14) if is_sphere(rec[k])] == [5, 9]
    lp = _check(rec, leaves)
    assert lp.tolist() == [[0, 4, 1], [10, 2, 0]]
    slots, _ = nh.pair_layout(rec, leaves)
    assert slots[:5].tolist() == [[0, 1], [2, 3], [4, 6], [7, 8], [5, 9]]
    assert slots[10:12].tolist() == [[10, 11], [12, 13]]
