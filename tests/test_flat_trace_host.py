"""The flat image of a scene whose tree is one leaf or a root with two leaves (host/gpu_layout.cpp flat_image, through
nh_flat_image): when a scene qualifies, and that the image holds the boxes, each leaf's pair counts and the pair records
of nh_pair_layout's arrangement by kind. CPU only.
"""
import itertools

import numpy as np
import pytest

import nori_hip as nh
import scenegen
from flat_trace_helpers import (HEADER_F4, MAX_PAIRS, PAIR_F4, as_int, expected_image, is_flat_tree, same_bits,
                                tree_boxes)
from pair_kind_helpers import leaf_table
from primary_mask_records import PRIM_SPHERE, device_records

ROOT = [-1.0, 0.0, -1.5, 1.0, 1.59, 1.0]
LEFT = [-1.0, 0.0, -1.5, 1.0, 1.25, 0.5]
RIGHT = [-0.5, 1.58, -0.25, 0.5, 1.59, 1.0]


def _records(kinds, seed=3):
    """(n, 12) float32 records with random vertices (a sphere: centre, radius), the kind bit beside other flag bits."""
    rng = np.random.default_rng(seed)
    rec = rng.uniform(-2, 2, (len(kinds), 12)).astype(np.float32)
    for k, sph in enumerate(kinds):
        rec[k, 11:12] = np.array([(PRIM_SPHERE | 8) if sph else (2 | 4)], np.int32).view(np.float32)
    return rec


def _check_flat(rec, leaves, boxes):
    img, eq = nh.flat_image(rec, leaves, boxes)
    assert img is not None
    want, want_eq = expected_image(rec, leaves, boxes)
    assert eq == want_eq and as_int(img[0, 3]) == eq and as_int(img[1, 3]) == len(leaves)
    assert img.shape == want.shape and (img.shape[0] - HEADER_F4) % PAIR_F4 == 0
    assert same_bits(img, want)
    return img, eq


@pytest.mark.parametrize("n", range(1, 11))
def test_single_leaf_every_mix_of_kinds(n):
    for kinds in itertools.product((False, True), repeat=n):
        rec = _records([False] + list(kinds) + [True], seed=n)  # (a record outside the leaf on each side)
        img, eq = _check_flat(rec, [(1, n)], ROOT + ROOT + ROOT)
        n_tri, n_sph = (kinds.count(False) + 1) // 2, (kinds.count(True) + 1) // 2
        assert eq == 1 and as_int(img[2, 3]) == n_tri | (n_sph << 16) and as_int(img[4, 3]) == 0
        assert len(img) == HEADER_F4 + PAIR_F4 * (n_tri + n_sph)
        assert same_bits(img[2, :3], img[0, :3]) and same_bits(img[3, :3], img[1, :3])  # the leaf's box is the root's


def test_two_leaves():
    rng = np.random.default_rng(11)
    for trial in range(100):
        nl, nr = int(rng.integers(1, 11)), int(rng.integers(1, 11))
        rec = _records(list(rng.random(nl + nr) < rng.choice([0.1, 0.5, 0.9])), seed=trial)
        img, eq = _check_flat(rec, [(0, nl), (nl, nr)], ROOT + LEFT + RIGHT)
        assert eq == 0
        assert same_bits(img[2, :3], LEFT[:3]) and same_bits(img[3, :3], LEFT[3:])
        assert same_bits(img[4, :3], RIGHT[:3]) and same_bits(img[5, :3], RIGHT[3:])


def test_box_equality_flag():
    rec = _records([False] * 6)
    leaves = [(0, 4), (4, 2)]
    assert _check_flat(rec, leaves, ROOT + ROOT + RIGHT)[1] == 1
    assert _check_flat(rec, leaves, ROOT + LEFT + ROOT)[1] == 2
    assert _check_flat(rec, leaves, ROOT + ROOT + ROOT)[1] == 3
    # equal as numbers, another bit pattern: not bit-equal
    zero_signs = list(ROOT)
    zero_signs[1] = -0.0
    assert _check_flat(rec, leaves, ROOT + zero_signs + RIGHT)[1] == 0


def test_three_leaves_are_not_flat():
    rec = _records([False] * 6)
    img, _ = nh.flat_image(rec, [(0, 2), (2, 2), (4, 2)], ROOT + LEFT + RIGHT)
    assert img is None


def test_seventeen_pair_positions_are_not_flat():
    """20 + 12 triangles: 10 + 6 = 16 pairs, flat; 20 + 13: 10 + 7 = 17, not. One leaf of 31 triangles and a sphere:
    16 + 1."""
    rec = _records([False] * 33)
    img, _ = _check_flat(rec, [(0, 20), (20, 12)], ROOT + LEFT + RIGHT)
    assert len(img) == HEADER_F4 + PAIR_F4 * MAX_PAIRS
    assert nh.flat_image(rec, [(0, 20), (20, 13)], ROOT + LEFT + RIGHT)[0] is None
    assert nh.flat_image(_records([False] * 31 + [True]), [(0, 32)], ROOT * 3)[0] is None
    assert nh.flat_image(_records([False] * 31), [(0, 31)], ROOT * 3)[0] is not None


def test_knob_and_caller_veto(monkeypatch):
    rec = _records([False, True, False])
    assert nh.flat_image(rec, [(0, 3)], ROOT * 3)[0] is not None
    assert nh.flat_image(rec, [(0, 3)], ROOT * 3, allowed=False)[0] is None  # not staged small / pairs not by kind
    monkeypatch.setenv("NH_FLAT_TRACE", "0")
    assert nh.flat_image(rec, [(0, 3)], ROOT * 3)[0] is None
    monkeypatch.setenv("NH_FLAT_TRACE", "1")
    assert nh.flat_image(rec, [(0, 3)], ROOT * 3)[0] is not None


def test_empty_and_invalid():
    assert nh.flat_image(np.zeros((0, 12), np.float32), [], ROOT * 3)[0] is None
    rec = _records([False] * 4)
    for leaves in ([(0, 5)], [(0, 3), (2, 2)], [(-1, 2)]):
        with pytest.raises(nh.NoriError):
            nh.flat_image(rec, leaves, ROOT * 3)


@pytest.mark.parametrize("variant", ["c1", "c2"])
def test_cornell_box(tmp_path, variant):
    """The Cornell box: a root and two leaves, 4 + 1 pairs and 2 pairs; the left child's box is bit-equal to the
    root's, the right child's (the ceiling slab) is not."""
    s = nh.Scene(scenegen.cbox_xml(str(tmp_path), variant))
    b = nh.Bvh(s)
    assert is_flat_tree(b) and leaf_table(b) == [(0, 10), (10, 4)]
    boxes = tree_boxes(b)
    img, eq = _check_flat(device_records(s, b), leaf_table(b), boxes)
    assert eq == 1
    assert same_bits(boxes[6:12], boxes[0:6]) and not same_bits(boxes[12:18], boxes[0:6])
    assert (as_int(img[2, 3]), as_int(img[4, 3])) == (4 | (1 << 16), 2)
    assert len(img) == HEADER_F4 + PAIR_F4 * 7
