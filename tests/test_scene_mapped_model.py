"""tests/scene_mapped_model.py on the CPU: the map and its composition, the per-sphere flag and snapshot tables, the two-pass edit list and
the refusal predicate of INTEGRATION.md section 21, on small hand-made tables with the answers written out."""
import numpy as np
import pytest

from tests import edit_influence_model as E
from tests import scene_mapped_model as S
from tests import scene_motion_model as M

DTYPES = [np.float32, np.float64]
CALL = "rtiow_edit_scene_mapped"


def tables(dt, n=5):
    return {"cr": np.array([[k, 0.5, -k, 0.5 + k] for k in range(n)], dt), "af": np.array([[0.125 * k, 0.25, 0.5, 0.0] for k in range(n)], dt),
            "ri": np.full(n, 1.5, dt), "ty": np.array([0, 1, 2, 0, 1][:n], np.int32)}


def rows(t, idx):
    return {key: np.ascontiguousarray(t[key][np.asarray(idx)]) for key in t}


def bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("dt", DTYPES)
def test_the_identity_map_is_sections_19_and_20(dt):
    snap = tables(dt)
    cur = tables(dt)
    cur["cr"][1, 0] += 0.25                                      # moved
    cur["af"][3, 2] = 0.75                                       # changed
    cur["cr"][4, 3] *= 2; cur["ty"][4] = 2                       # both
    fs = S.identity(5)
    assert S.flags(cur, snap, fs).tolist() == M.flags(cur, snap).tolist() == [0, 1, 0, 2, 3]
    assert bits(S.snap_table(cur, snap, fs)) == bits(snap["cr"])
    got, want = S.edit_list(cur, snap, fs), E.edit_list(cur, snap)
    assert bits(got[0]) == bits(want[0]) and got[1].tolist() == want[1].tolist() == [1, 1, 3, 4, 4]
    al = S.aligned(cur, snap, fs)
    assert all(bits(al[key]) == bits(snap[key]) for key in snap)


def test_composition_over_two_and_three_edits():
    # the committed scene: 6 slots, slot 2 dropped: kept slots 0 1 3 4 5 are spheres 0..4 of the snapshot
    kept0 = np.array([1, 1, 0, 1, 1, 1])
    fs0 = S.identity(5)
    # edit 1: 5 slots: slot 5, a new sphere, slot 0, a dropped slot (its origin is not read), slot 3
    kept1, origin1 = np.array([1, 1, 1, 0, 1]), np.array([5, -1, 0, 99, 3])
    fs1 = S.compose(fs0, kept0, kept1, origin1)
    assert fs1.tolist() == [4, -1, 0, 2]                         # slot 5 is sphere 4, slot 0 sphere 0, slot 3 sphere 2; spheres 1 and 3 are removed
    # edit 2, no commit between: the new sphere is continued (moved, say), slot 4 (sphere 2 of the snapshot) too, one more is added
    kept2, origin2 = np.array([1, 1, 1]), np.array([1, 4, -1])
    fs2 = S.compose(fs1, kept1, kept2, origin2)
    assert fs2.tolist() == [-1, 2, -1]                           # added then moved: still no origin
    # edit 3: a permutation of edit 2's slots with one dropped
    kept3, origin3 = np.array([1, 0, 1]), np.array([2, 0, 1])
    assert S.compose(fs2, kept2, kept3, origin3).tolist() == [-1, 2]
    # an edit that keeps every slot where it is composes to the same map
    assert S.compose(fs1, kept1, kept1, np.arange(5)).tolist() == fs1.tolist()


@pytest.mark.parametrize("dt", DTYPES)
def test_tables_and_two_pass_list_of_a_mapped_edit(dt):
    snap = tables(dt)
    # current scene: snapshot sphere 3 recoloured, an added sphere, snapshot sphere 0 untouched, snapshot sphere 4 moved; 1 and 2 are removed
    cur = rows(snap, [3, 0, 0, 4])
    cur["af"][0, 0] = 0.875
    cur["cr"][1] = [9, 9, 9, 0.25]
    cur["cr"][3, :3] += 0.5
    fs = np.array([3, -1, 0, 4], np.int32)
    assert S.flags(cur, snap, fs).tolist() == [M.CHANGED, M.CHANGED, 0, M.MOVED]
    table = S.snap_table(cur, snap, fs)
    assert bits(table[0]) == bits(snap["cr"][3]) and bits(table[2]) == bits(snap["cr"][0]) and bits(table[3]) == bits(snap["cr"][4])
    assert bits(table[1]) == bits(np.zeros(4, dt))
    entries, owners = S.edit_list(cur, snap, fs)
    assert owners.tolist() == [0, 1, 3, 3, S.OWNER_REMOVED, S.OWNER_REMOVED]
    want = [cur["cr"][0], cur["cr"][1], snap["cr"][4], cur["cr"][3], snap["cr"][1], snap["cr"][2]]
    assert bits(entries) == bits(np.array(want, dt)) and entries.dtype == dt
    # the aligned snapshot says the same through section 19's comparison: CHANGED outranks MOVED at the added sphere
    f19 = M.flags(cur, S.aligned(cur, snap, fs))
    assert ((f19 & M.CHANGED) != 0).tolist() == [True, True, False, False] and ((f19 & ~M.CHANGED) != 0).tolist()[2:] == [False, True]
    # an added sphere that repeats a snapshot record bit for bit is still added
    twin = rows(snap, [0, 0])
    assert S.flags(twin, snap, np.array([0, -1])).tolist() == [0, M.CHANGED]


@pytest.mark.parametrize("dt", DTYPES)
def test_added_then_removed_leaves_no_entry(dt):
    snap = tables(dt, 3)
    kept0, fs0 = np.ones(3), S.identity(3)
    kept1, origin1 = np.ones(4), np.array([0, 1, 2, -1])         # add one
    fs1 = S.compose(fs0, kept0, kept1, origin1)
    assert fs1.tolist() == [0, 1, 2, -1]
    kept2, origin2 = np.ones(3), np.array([0, 1, 2])             # ... and take it away again before any commit
    fs2 = S.compose(fs1, kept1, kept2, origin2)
    assert fs2.tolist() == [0, 1, 2]
    entries, owners = S.edit_list(tables(dt, 3), snap, fs2)
    assert len(owners) == 0 and entries.shape == (0, 4)
    # pass 2 is in the snapshot's order whatever the current order is
    cur = rows(snap, [1])
    assert S.edit_list(cur, snap, np.array([1]))[1].tolist() == [S.OWNER_REMOVED] * 2
    assert bits(S.edit_list(cur, snap, np.array([1]))[0]) == bits(snap["cr"][[0, 2]])


def test_the_refusal_predicate_and_its_order():
    kept = np.array([1, 1, 0, 1])
    ty = [0, 1, 2, 0, 1]
    ok = dict(tables=True, n=3, valid=None, types=ty, origin=[0, -1, 3], have_scene=True, current_kept=kept)
    assert S.refusal(CALL, **ok) == (0, "")
    ask = lambda **kw: S.refusal(CALL, **dict(ok, **kw))
    assert ask(tables=False, have_scene=False, origin=None) == (S.E_BADARG, CALL + ": null or empty table")
    assert ask(n=0, have_scene=False) == (S.E_BADARG, CALL + ": null or empty table") and ask(n=-2)[0] == S.E_BADARG
    assert ask(have_scene=False, origin=None) == (S.E_STATE, CALL + " before rtiow_set_scene")
    assert ask(origin=None, types=[7, 7, 7]) == (S.E_BADARG, CALL + ": origin must not be NULL (-1 per slot: every sphere is new)")
    slot = CALL + ": origin must be -1 or a slot the current scene keeps"
    for bad in ([0, -2, 3], [0, 4, 3], [0, 2, 3], [0, 1 << 30, 3]):
        assert ask(origin=bad) == (S.E_BADARG, slot), bad
    assert ask(origin=[0, 0, 4]) == (S.E_BADARG, slot)           # range before duplicates
    twice = CALL + ": two slots continue the same sphere (a sphere is continued at most once)"
    assert ask(origin=[0, 0, 3], types=[0, 9, 0]) == (S.E_BADARG, twice)   # duplicates before the type
    assert ask(origin=[-1, -1, -1]) == (0, "")                   # -1 may repeat
    assert ask(types=[0, 3, 0]) == (S.E_BADARG, "material type out of range") and ask(types=[0, -1, 0])[0] == S.E_BADARG
    # a dropped slot is not read: neither its origin nor its type
    assert ask(valid=[1, 0, 1], origin=[0, 77, 3], types=[0, 9, 0]) == (0, "")
    assert ask(valid=[1, 0, 1], origin=[0, 0, 3]) == (0, "")
    assert ask(valid=[0, 0, 0]) == (S.E_BADARG, "scene has no valid spheres")
    assert ask(n=5, origin=[0, 1, 3, -1, -1]) == (0, "")         # any n


def test_the_edit_helpers_give_scenes_with_their_origin():
    scene = {"scene_id": 0, "precision": 32, "center_radius": np.arange(16, dtype=np.float32).reshape(4, 4), "albedo_fuzz": np.zeros((4, 4), np.float32),
             "refraction_index": np.ones(4, np.float32), "type": np.array([0, 1, 2, 0], np.int32), "valid": np.array([1, 1, 0, 1], np.int32)}
    out, origin = S.take(scene, [3, 0, 2])
    assert origin.tolist() == [3, 0, 2] and out["valid"].tolist() == [1, 1, 0] and out["center_radius"][0, 0] == 12 and len(scene["type"]) == 4
    out, origin = S.drop(scene, [1])
    assert origin.tolist() == [0, 1, 2, 3] and out["valid"].tolist() == [1, 0, 0, 1] and scene["valid"].tolist() == [1, 1, 0, 1]
    out, origin = S.append(scene, [[1, 2, 3, 0.5]] * 2, [[0.5, 0.5, 0.5, 0]] * 2, [1.5, 1.5], [0, 2])
    assert origin.tolist() == [0, 1, 2, 3, -1, -1] and out["type"].tolist() == [0, 1, 2, 0, 0, 2] and out["center_radius"].dtype == np.float32
    assert S.then([3, 0, 2], [1, -1, 0]).tolist() == [0, -1, 3]
    assert S.compose(S.identity(3), S.kept_pattern(scene), S.kept_pattern(S.take(scene, [3, 0, 2])[0]), [3, 0, 2]).tolist() == [2, 0]
    assert S.same_slots(scene).tolist() == [0, 1, 2, 3] and S.kept_pattern(dict(scene, valid=None)).tolist() == [1, 1, 1, 1]
