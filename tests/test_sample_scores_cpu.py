"""CPU: the restatement tests/sample_scores_ref.py against hand-worked cases (a query on a bank row, on a ball's boundary, inside
no ball, inside two balls; pruning with tied radii, all pruned but one, all pruned); what the shared cases of the GPU tests
contain, shown on the reference alone; the argument errors of common/sample_scores.py; and the refusals of the two C entry
points (csrc/prd.hip), decided on the host before anything is launched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prd_ref  # noqa: E402
import sample_scores_ref as S  # noqa: E402

INF = np.inf


def test_hand_worked_scores():
    bank = np.array([[0, 0], [10, 0], [0, 10]], np.float32)
    radii2 = np.array([25.0, 4.0, 0.0])
    queries = np.array([[0, 0],        # on bank row 0: d2 == 0 -> +inf; only ball 0 holds it
                        [3, 4],        # on the boundary of ball 0: 25 / 25 == 1, and the boundary belongs to the ball
                        [6, 0],        # inside no ball: 25 / 36 from row 0, 4 / 16 from row 1, 0 / 136 from row 2
                        [0, 10]],      # on bank row 2, whose radius is 0: 0 / 0 counts as +inf, and the ball {row 2} holds it
                       np.float32)
    ratio2, rare2 = S.scores2(queries, bank, radii2)
    assert ratio2.tolist() == [INF, 1.0, 25.0 / 36.0, INF]
    assert rare2.tolist() == [25.0, 25.0, INF, 0.0]
    # inside two balls: the smaller one is the rarity, the larger ratio the realism
    ratio2, rare2 = S.scores2(np.array([[9, 0]], np.float32), bank, np.array([121.0, 4.0, 0.0]))
    assert ratio2.tolist() == [4.0] and rare2.tolist() == [4.0]             # 121 / 81 < 4 / 1; min(121, 4)
    # a pruned ball takes part in neither value
    ratio2, rare2 = S.scores2(np.array([[9, 0]], np.float32), bank, np.array([121.0, -1.0, 0.0]))
    assert ratio2.tolist() == [121.0 / 81.0] and rare2.tolist() == [121.0]
    ratio2, rare2 = S.scores2(queries, bank, np.array([-1.0, -1.0, -1.0]))
    assert ratio2.tolist() == [-INF] * 4 and rare2.tolist() == [INF] * 4


def test_pruning_ties_go_to_the_lowest_index():
    radii2 = np.array([4.0, 1.0, 4.0, 4.0, 9.0, 1.0])
    assert S.prune_radii(radii2, 0.5).tolist() == [4.0, 1.0, -1.0, -1.0, -1.0, 1.0]        # keeps 1, 5 and the FIRST of the 4s
    assert S.prune_radii(radii2, 0.0).tolist() == radii2.tolist()
    assert S.prune_radii(radii2, 0.4).tolist() == [4.0, 1.0, 4.0, -1.0, -1.0, 1.0]         # ceil(3.6) = 4
    assert S.prune_radii(radii2, 0.99).tolist() == [-1.0, 1.0, -1.0, -1.0, -1.0, -1.0]     # all but one: the first of the 1s
    assert radii2.tolist() == [4.0, 1.0, 4.0, 4.0, 9.0, 1.0]                               # the input is not touched
    bank = np.arange(6, dtype=np.float32)[:, None] * np.float32(2)                         # 0, 2, .., 10 on a line
    ratio2, rare2 = S.scores2(np.array([[3.0]], np.float32), bank, S.prune_radii(radii2, 0.99))
    assert ratio2.tolist() == [1.0] and rare2.tolist() == [1.0]                            # only row 1 (at 2): 1 / 1, on its boundary


def test_hand_worked_through_the_radii():
    real = np.array([[0], [1], [3], [7]], np.float32)          # 1-NN radii2: 1, 1, 4, 16
    assert prd_ref.radii(real, 1).tolist() == [1.0, 1.0, 4.0, 16.0]
    fake = np.array([[2], [20]], np.float32)                   # d2 of 2: 4, 1, 1, 25; of 20: 400, 361, 289, 169
    assert S.realism(real, fake, 1, prune=0.0).tolist() == [2.0, np.sqrt(16.0 / 169.0)]     # 4 / 1 from row 2; 16 / 169
    assert S.realism(real, fake, 1, prune=0.5).tolist() == [1.0, np.sqrt(1.0 / 361.0)]      # rows 0 and 1 stay: 1 / 1; 1 / 361
    score, inside = S.rarity(real, fake, 1)
    assert score.tolist() == [1.0, 0.0] and inside.tolist() == [True, False]                # balls 1 and 2 hold it: min(1, 4)
    got = S.sample_scores(real, fake, 1, prune=0.0)
    assert got['mean_realism'] == (2.0 + np.sqrt(16.0 / 169.0)) / 2 and got['realistic_fraction'] == 0.5 and got['mean_rarity'] == 1.0
    assert np.isnan(S.sample_scores(real, fake[1:], 1)['mean_rarity'])


@pytest.mark.parametrize("d,nq,nr,k", S.exact_cases())
def test_the_exact_cases_hold_what_the_gpu_tests_need(d, nq, nr, k):
    e = S.exact_case(d, nq, nr, k)
    T = S.tile_width()
    assert nr in (T - 1, 2 * T + 1) and np.abs(e['q']).max() <= 3 and np.abs(e['r']).max() <= 3
    d2 = prd_ref.d2(e['q'], e['r'])
    assert np.array_equal(d2, np.round(d2)) and np.array_equal(e['radii2'], np.round(e['radii2']))      # exact integers
    assert np.array_equal(d2, prd_ref.integer_d2(e['q'].astype(np.int64), e['r'].astype(np.int64)).astype(np.float64))
    assert e['ratio2'][0] == INF and d2[0, 2] == 0                                   # a query copied from a bank row
    if k == 1:
        assert e['radii2'][2] == e['radii2'][5] == e['radii2'][nr - 1] == 0.0        # duplicated bank rows: radius 0, 0 / 0 -> +inf
    assert (e['pruned2'] < 0).sum() == nr - (nr + 1) // 2
    if nq > 8:
        nearest = d2.argmin(axis=1)
        assert e['pruned2'][nearest[7]] < 0 and d2[7, nearest[7]] == 0 and e['ratio2'][7] == INF and e['ratio2_pruned'][7] < INF
        assert (e['ratio2_pruned'] < e['ratio2']).sum() >= 1
        assert 0 < e['inside'].sum() < nq                                            # both kinds of row
        assert (d2 == e['radii2'][None, :]).sum() >= 1                               # pairs ON a boundary: inclusive matters


def test_the_gaussian_case_sets_no_row_aside():
    """what lets the GPU test demand rare2 == the restatement on EVERY row (its cap is 1 % of the rows), and the premise
    A_ij <= 2 d2_ij of sample_scores_ref.ratio_rel_bound"""
    g = S.gaussian_case()
    assert g['q'].shape == (130, 2048) and g['r'].shape == (200, 2048)
    assert S.undecided_rows(g['q'], g['r'], g['radii2']).sum() == 0
    d2, bound = prd_ref.d2(g['q'], g['r']), prd_ref.d2_bound(g['q'], g['r'])
    assert np.all(bound / (2 * (2048 + 4) * 2.0 ** -53) <= 2 * d2)
    inside = np.isfinite(g['rare2'])
    print(f"inside {int(inside.sum())} of {len(inside)}, with the pruned balls {int(np.isfinite(g['rare2_pruned']).sum())}, "
          f"bound on ratio2 {S.ratio_rel_bound(2048):.3g}")
    assert 0 < inside.sum() < len(inside) and np.all(np.isfinite(g['ratio2']))


def test_argument_errors():
    from gan_lib_tensorflow_amd.common import sample_scores as SS
    few, many = np.zeros((3, 2048), np.float32), np.zeros((8, 2048), np.float32)
    for prune in (1.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match="prune"):
            SS.realism_scores(many, many, prune=prune)
        with pytest.raises(ValueError, match="prune"):
            SS.calculate_sample_scores(many, many, prune=prune)
    with pytest.raises(ValueError, match="at least 4"):
        SS.realism_scores(few, many)
    with pytest.raises(ValueError, match="at least 4"):
        SS.rarity_scores(few, many)
    with pytest.raises(ValueError, match="at least 4"):
        SS.calculate_sample_scores(few, many)
    with pytest.raises(ValueError, match="k = 9"):
        SS.rarity_scores(many, many, k=9)
    with pytest.raises(ValueError, match="no rows"):
        SS.rarity_scores(many, many[:0])
    images = np.zeros((8, 32, 32, 3), np.uint8)
    for fn in (SS.realism_scores, SS.rarity_scores, SS.calculate_sample_scores):
        with pytest.raises(NotImplementedError, match="needs downloaded weights"):
            fn(images, many)
        with pytest.raises(NotImplementedError, match="needs downloaded weights"):
            fn(many, images)
        with pytest.raises(TypeError):
            fn("features.npy", many)


def test_rank_samples():
    from gan_lib_tensorflow_amd.common import sample_scores as SS
    scores = np.array([1.0, INF, 0.5, 1.0, 0.0, INF])
    got = SS.rank_samples(scores, 4)
    assert got.dtype == np.int64 and got.tolist() == [1, 5, 0, 3]                 # ties to the lowest index
    assert SS.rank_samples(scores, 3, largest=False).tolist() == [4, 2, 0]
    assert SS.rank_samples(scores, 0).tolist() == [] and SS.rank_samples(scores, 6).tolist() == [1, 5, 0, 3, 2, 4]
    with pytest.raises(ValueError, match="n = 7"):
        SS.rank_samples(scores, 7)
    with pytest.raises(ValueError, match="NaN"):
        SS.rank_samples(np.array([1.0, np.nan]), 1)
    with pytest.raises(ValueError, match=r"expected \[N\]"):
        SS.rank_samples(np.zeros((2, 2)), 1)


def entry_points_refuse(lib):
    """every call is refused by the argument checks: the pointers are never dereferenced and nothing is launched"""
    fake = C.c_void_p(0x1000)

    def err():
        return lib.gank_last_error().decode()

    def partial(q=fake, nq=100, r=fake, nr=100, d=64, radii2=fake, segments=1, part_ratio2=fake, part_rare2=fake):
        return lib.gank_prd_scores_partial(q, nq, r, nr, d, radii2, segments, part_ratio2, part_rare2, None)

    for name in ("q", "r", "radii2", "part_ratio2", "part_rare2"):
        assert partial(**{name: None}) != 0 and "prd_scores_partial: null pointer" in err()
    assert partial(d=24) != 0 and "D = 24 unsupported" in err()
    assert partial(d=8) != 0 and "unsupported" in err()
    assert partial(d=4112) != 0 and "unsupported" in err()
    assert partial(nq=0) != 0 and "nq = 0" in err()
    assert partial(nr=0) != 0 and "nr = 0" in err()
    assert partial(segments=0) != 0 and "segments = 0" in err()
    assert partial(nq=1000, segments=3) != 0 and "segments = 3" in err() and "2 column tiles" in err()      # the BANK's tiles
    assert partial(nq=(1 << 24) + 1) != 0 and "nq =" in err()
    assert partial(q=C.c_void_p(0x1008)) != 0 and "misaligned" in err()                # features: 16 bytes
    assert partial(r=C.c_void_p(0x1004)) != 0 and "misaligned" in err()
    assert partial(radii2=C.c_void_p(0x1004)) != 0 and "misaligned" in err()

    def finish(part_ratio2=fake, part_rare2=fake, nq=100, segments=1, ratio2=fake, rare2=fake):
        return lib.gank_prd_scores_finish(part_ratio2, part_rare2, nq, segments, ratio2, rare2, None)

    for name in ("part_ratio2", "part_rare2", "ratio2", "rare2"):
        assert finish(**{name: None}) != 0 and "prd_scores_finish: null pointer" in err()
    assert finish(nq=0) != 0 and "nq = 0" in err()
    assert finish(segments=0) != 0 and "segments = 0" in err()
    assert finish(segments=65536) != 0 and "segments = 65536" in err()


def test_entry_points_refuse_bad_arguments_with_a_message():
    from gan_lib_tensorflow_amd import _lib
    entry_points_refuse(_lib.load())
