"""Scene edits that add and remove spheres (rtiow_edit_scene_mapped): the numpy restatement of INTEGRATION.md section 21, on top of
tests/scene_motion_model.py (section 19) and tests/edit_influence_model.py (section 20), which it imports and does not edit.  Pure numpy.

The map.  from_snapshot[k] per kept sphere k of the current scene: the number j of the sphere it continues among the kept spheres of the
snapshot, or -1.  A commit makes it the identity.  A mapped edit with origin[i] per slot i of the new scene (the slot of the CURRENT scene
that slot i continues, or -1) composes it: for kept slot i, numbered k', from_snapshot'[k'] = -1 where origin[i] == -1, else
from_snapshot[k] for the number k of slot origin[i] among the current scene's kept slots.

The tables.  Per kept sphere k with j = from_snapshot[k]: j >= 0: MOVED / CHANGED from the current record of k against snapshot record
j, bits against bits, and {C'_j, r'_j}; j == -1: CHANGED alone and four zeros of T.

The edit list, in two passes.  Pass 1, the current scene's kept spheres in ascending k, owner k: MOVED: {C'_j, r'_j}, then {C_k, r_k};
CHANGED only (an added sphere is this case): {C_k, r_k}; neither: none.  Pass 2, the snapshot's spheres j in ascending order that no
current sphere continues: {C'_j, r'_j} with the owner -2.

The plane, the gathers and lambda are sections 19 and 20 over these tables: aligned() lays the snapshot out in the current numbering and
hands it to scene_motion_model.plane_np; edit_influence_model.influence_np takes the two-pass list as it is (no pixel's id is -2).
tests/test_scene_mapped_model.py pins these functions on the CPU."""
import numpy as np

from tests import edit_influence_model as E
from tests import scene_motion_model as M

NO_ORIGIN, OWNER_REMOVED = -1, -2
E_BADARG, E_STATE = -1, -2
KEYS = ("center_radius", "albedo_fuzz", "refraction_index", "type", "valid")


# ---- the map

def identity(spheres):
    return np.arange(spheres, dtype=np.int32)


def kept_pattern(scene):
    """1 per slot the scene keeps, 0 per slot it drops."""
    n = len(scene["type"])
    return (np.asarray(scene["valid"]) != 0).astype(np.int32) if scene.get("valid") is not None else np.ones(n, np.int32)


def compose(from_snapshot, current_kept, new_kept, origin):
    """from_snapshot' after a mapped edit: current_kept / new_kept are kept_pattern() of the scene the handle holds and of the new one."""
    number = np.cumsum(np.asarray(current_kept) != 0) - 1        # slot of the current scene -> its number among the kept
    out = []
    for i in np.flatnonzero(np.asarray(new_kept) != 0):
        out.append(NO_ORIGIN if origin[i] < 0 else int(from_snapshot[number[origin[i]]]))
    return np.array(out, np.int32)


def refusal(call, tables, n, valid, types, origin, have_scene, current_kept):
    """(code, text) of the argument checks of rtiow_edit_scene_mapped behind the NULL handle, in the order it asks; (0, "") accepts.
    current_kept: kept_pattern() of the scene the handle holds (its length is the current slot count)."""
    if not tables or n <= 0:
        return E_BADARG, call + ": null or empty table"
    if not have_scene:
        return E_STATE, call + " before rtiow_set_scene"
    if origin is None:
        return E_BADARG, call + ": origin must not be NULL (-1 per slot: every sphere is new)"
    keeps = [valid is None or valid[i] != 0 for i in range(n)]
    for i in range(n):
        if keeps[i] and origin[i] != -1 and (origin[i] < -1 or origin[i] >= len(current_kept) or not current_kept[origin[i]]):
            return E_BADARG, call + ": origin must be -1 or a slot the current scene keeps"
    named = [int(origin[i]) for i in range(n) if keeps[i] and origin[i] >= 0]
    if len(set(named)) != len(named):
        return E_BADARG, call + ": two slots continue the same sphere (a sphere is continued at most once)"
    for i in range(n):
        if keeps[i] and not 0 <= types[i] <= 2:
            return E_BADARG, "material type out of range"
    if not any(keeps):
        return E_BADARG, "scene has no valid spheres"
    return 0, ""


# ---- the per-sphere tables (cur, snap: M.tables)

def flags(cur, snap, from_snapshot):
    out = np.zeros(len(cur["ty"]), np.int64)
    for k, j in enumerate(from_snapshot):
        if j < 0:
            out[k] = M.CHANGED
            continue
        one = lambda t, at: {key: t[key][at:at + 1] for key in ("cr", "af", "ri", "ty")}
        out[k] = M.flags(one(cur, k), one(snap, int(j)))[0]
    return out


def snap_table(cur, snap, from_snapshot):
    """[spheres, 4] in T: {C'_j, r'_j} per kept sphere of the current scene, zeros for an added one."""
    out = np.zeros_like(cur["cr"])
    for k, j in enumerate(from_snapshot):
        if j >= 0:
            out[k] = snap["cr"][int(j)]
    return out


def edit_list(cur, snap, from_snapshot):
    """(entries [E, 4] in T, owners [E] int32): pass 1 over the current scene, pass 2 over the snapshot's removed spheres."""
    entries, owners = [], []
    for k, f in enumerate(flags(cur, snap, from_snapshot)):
        if f & M.MOVED:
            entries += [snap["cr"][int(from_snapshot[k])], cur["cr"][k]]
            owners += [k, k]
        elif f & M.CHANGED:
            entries.append(cur["cr"][k])
            owners.append(k)
    continued = set(int(j) for j in from_snapshot if j >= 0)
    for j in range(len(snap["ty"])):
        if j not in continued:
            entries.append(snap["cr"][j])
            owners.append(OWNER_REMOVED)
    return np.array(entries, cur["cr"].dtype).reshape(-1, 4), np.array(owners, np.int32)


def aligned(cur, snap, from_snapshot):
    """The snapshot laid out in the current scene's numbering, for scene_motion_model.plane_np: record j of the snapshot at k, and at an
    added sphere zeros with a type no material has, so that the comparison says CHANGED there (which outranks MOVED in the plane)."""
    out = {"cr": snap_table(cur, snap, from_snapshot), "af": np.zeros_like(cur["af"]), "ri": np.zeros_like(cur["ri"]),
           "ty": np.full_like(cur["ty"], -1)}
    for k, j in enumerate(from_snapshot):
        if j >= 0:
            for key in ("af", "ri", "ty"):
                out[key][k] = snap[key][int(j)]
    return out


def planes(oracle, prec, scene, cam, snap, from_snapshot, kappa, rows=None):
    """The model's planes of `scene` at `cam` against the snapshot through the map: the motion plane, the guides, the list and lambda.
    kappa == 0 (off) gives lambda = 0 and fade = carry, with which edit_influence_model's gathers are section 19's bit for bit."""
    cur = M.tables(scene, prec)
    rows = range(cam.img_height) if rows is None else rows
    O, D, t, k = M.first_hit(oracle, prec, cur, cam, rows)
    Q, carry, ids = M.plane_np(O, D, t, k, cur, aligned(cur, snap, from_snapshot))
    normal, depth = M.guides_of(O, D, t, k, cur)
    entries, owners = edit_list(cur, snap, from_snapshot)
    lam, fade, s = E.influence_np(cam, depth, carry, ids, entries, owners, kappa, rows)
    return {"Q": Q, "carry": carry, "ids": ids, "N": normal, "t": depth, "entries": entries, "owners": owners, "lam": lam, "fade": fade, "s": s}


# ---- edited scenes with their origin: functions of a scene dict returning (scene', origin), origin in the slots of the scene passed in

def with_valid(scene):
    return dict(M.edited(scene), valid=kept_pattern(scene))


def take(scene, slots):
    """The slots of `scene` in the order given: a permutation, or a scene without some slots (n changes)."""
    slots = np.asarray(slots, np.int64)
    out = with_valid(scene)
    for key in KEYS:
        out[key] = np.ascontiguousarray(out[key][slots])
    return out, slots.astype(np.int32)


def drop(scene, slots):
    """The same slots with `slots` marked invalid (n stays)."""
    out = with_valid(scene)
    out["valid"][np.asarray(slots, np.int64)] = 0
    return out, np.arange(len(out["type"]), dtype=np.int32)


def append(scene, center_radius, albedo_fuzz, refraction_index, types):
    """`scene` with new spheres in new slots behind it."""
    out = with_valid(scene)
    more = {"center_radius": np.asarray(center_radius, out["center_radius"].dtype).reshape(-1, 4),
            "albedo_fuzz": np.asarray(albedo_fuzz, out["albedo_fuzz"].dtype).reshape(-1, 4),
            "refraction_index": np.asarray(refraction_index, out["refraction_index"].dtype).reshape(-1),
            "type": np.asarray(types, np.int32).reshape(-1)}
    more["valid"] = np.ones(len(more["type"]), np.int32)
    n = len(out["type"])
    for key in KEYS:
        out[key] = np.ascontiguousarray(np.concatenate([out[key], more[key]]))
    return out, np.concatenate([np.arange(n), np.full(len(more["type"]), NO_ORIGIN)]).astype(np.int32)


def same_slots(scene):
    """The origin of an edit that keeps every slot where it is (what rtiow_edit_scene assumes)."""
    return np.arange(len(scene["type"]), dtype=np.int32)


def then(first, second):
    """The origin of two steps in one call: `first` maps the middle scene's slots to the start's, `second` the end's to the middle's."""
    first, second = np.asarray(first), np.asarray(second)
    return np.where(second < 0, NO_ORIGIN, first[np.maximum(second, 0)]).astype(np.int32)
