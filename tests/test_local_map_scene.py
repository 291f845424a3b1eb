"""tests/local_map_scene.py against itself, without a GPU: the table definitions of dvm_update_local_map_keyframes / _points in numpy
(what the device computes) equal the reference's two loops restated statement by statement, on seeded graphs that hold every case the
issue names -- a point held by two keypoints of the frame, bad points in the frame and in rows, a queued keyframe (matches set, no
observation), a point in several rows, a frame point in no row.  All comparisons are integer equality."""
import numpy as np
import pytest

import local_map_scene as lms


def _graph(seed, queued=(), **kw):
    a = dict(kf_slots=[3, 0, 7, 12, 5], row_lens=[40, 0, 65, 17, 64], n_points=90, frame_n=70, map_capacity=200, kf_capacity=16, slot_keypoints=80,
             queued=queued)
    a.update(kw)
    return lms.make_graph(seed, **a)


def _tables(g, kf_order):
    obs = {kf.slot: lms.row_observed(kf, g.points) for kf in g.kfs}
    mat = {kf.slot: lms.row_matches(kf) for kf in g.kfs}
    votes, frame_bad = lms.votes_table(g.frame_slots(), g.bad_table(), obs, g.kf_capacity)
    local = lms.local_points_table([kf.slot for kf in kf_order], mat, g.bad_table(), g.frame_slots())
    return votes, frame_bad, local, obs, mat


@pytest.mark.parametrize("seed", range(8))
def test_tables_equal_the_loops(seed):
    g = _graph(seed, queued=(2,) if seed % 2 else ())
    rng = np.random.default_rng(100 + seed)
    order = [g.kfs[i] for i in rng.permutation(len(g.kfs))[:1 + seed % len(g.kfs)]]
    votes, frame_bad, (local_slot, frame_mp, n_outside), _, _ = _tables(g, order)
    r_votes, r_bad = lms.reference_keyframes(g)
    r_local, r_mp, r_out = lms.reference_points(g, order)
    assert np.array_equal(votes, r_votes) and np.array_equal(frame_bad, r_bad)
    assert np.array_equal(local_slot, r_local) and np.array_equal(frame_mp, r_mp) and n_outside == r_out


def test_the_seeded_graphs_hold_the_named_cases():
    g = _graph(1, queued=(2,))
    fs = g.frame_slots()
    bad = g.bad_table()
    held, counts = np.unique(fs[fs >= 0], return_counts=True)
    assert (counts[~bad[held]] >= 2).any(), "a non-bad point held by two keypoints of the frame"
    assert bad[fs[fs >= 0]].any(), "a bad point in the frame"
    rows = [lms.row_matches(kf) for kf in g.kfs]
    assert any(bad[r[r >= 0]].any() for r in rows), "a bad point in a row"
    in_rows = np.concatenate([np.unique(r[r >= 0]) for r in rows])
    assert (np.unique(in_rows, return_counts=True)[1] >= 2).any(), "a point in several rows"
    assert any(((r[r >= 0][:, None] == r[r >= 0][None, :]).sum(1) >= 2).any() for r in rows if (r >= 0).any()), "a repeat inside one row"
    live = fs[(fs >= 0)]
    live = live[~bad[live]]
    assert (~np.isin(live, in_rows)).any(), "a live frame point in no row"
    assert any(len(kf.matches) == 0 for kf in g.kfs), "a row of length 0"


def test_a_point_held_twice_votes_twice():
    g = _graph(3)
    p = next(q for q in g.points if not q.bad and q.observations)
    g.frame = [p, None, p]
    votes, frame_bad = lms.reference_keyframes(g)
    for kf in g.kfs:
        assert votes[kf.slot] == (2 if kf in p.observations else 0)
    t_votes, t_bad, _, _, _ = _tables(g, g.kfs)
    assert np.array_equal(t_votes, votes) and np.array_equal(t_bad, frame_bad) and not frame_bad.any()


def test_the_queued_keyframe_needs_both_rows():
    """A keyframe whose matches are set and whose observations are not: it receives no votes, and its points are listed.  One table for
    both walks is wrong on this graph either way."""
    g = _graph(5, queued=(2,), bad_frac=0.0)
    q = g.kfs[2]
    only_q = [p for p in q.matches if p is not None and not p.observations]
    assert only_q, "the queued keyframe holds a point nobody observes yet"
    g.frame = [p for p in q.matches if p is not None][:20]
    votes, frame_bad, (local_slot, frame_mp, n_outside), obs, mat = _tables(g, g.kfs)
    r_votes, _ = lms.reference_keyframes(g)
    r_local, r_mp, r_out = lms.reference_points(g, g.kfs)
    assert np.array_equal(votes, r_votes) and votes[q.slot] == 0
    assert np.array_equal(local_slot, r_local) and np.array_equal(frame_mp, r_mp) and n_outside == r_out == 0
    assert only_q[0].slot in local_slot
    # MATCHES used for the votes: the queued keyframe is voted for
    wrong_votes, _ = lms.votes_table(g.frame_slots(), g.bad_table(), mat, g.kf_capacity)
    assert wrong_votes[q.slot] > 0 and not np.array_equal(wrong_votes, r_votes)
    # OBSERVED used for the local points: the queued keyframe's own points are missing
    wrong_local, _, wrong_out = lms.local_points_table([kf.slot for kf in g.kfs], obs, g.bad_table(), g.frame_slots())
    assert only_q[0].slot not in wrong_local and not np.array_equal(wrong_local, r_local)


def test_degenerate_graphs():
    for kw in (dict(frame_n=0), dict(fill=0.0), dict(bad_frac=1.0), dict(kf_slots=[], row_lens=[]), dict(n_points=0)):
        g = _graph(9, **kw)
        votes, frame_bad, (local_slot, frame_mp, n_outside), _, _ = _tables(g, g.kfs)
        r_votes, r_bad = lms.reference_keyframes(g)
        r_local, r_mp, r_out = lms.reference_points(g, g.kfs)
        assert np.array_equal(votes, r_votes) and np.array_equal(frame_bad, r_bad)
        assert np.array_equal(local_slot, r_local) and np.array_equal(frame_mp, r_mp) and n_outside == r_out
