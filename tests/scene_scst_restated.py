"""Self-critical training over every matched object of a scene restated in numpy: the specification of
``spacap_scst_select_f32`` (csrc/scst_select.hip) and of ``spacap_caption_prep_rows_fwd_f32`` / ``_bwd_f32``
(csrc/caption_prep.hip), with the inputs both test modules run through them.  Not a test module.  Rewards, advantages and the
loss are those of tests/self_critical_restated.py with groups in the place of scenes.

Selection.  Object slot j of scene b is a candidate when box_label_mask[b,j] > 0 and it has a key row (``SC.key_row``).  Its
proposal is the first minimum over k of d = ((x - cx)^2 + (z - cz)^2) + (y - cy)^2 in float32, each operation rounded (no
contraction); a NaN distance is never a minimum, an object without a finite minimum does not qualify, and it qualifies when
d < near2 = float32(near) * float32(near), strictly.  The qualifying objects in (d, j) order fill the first slots, M at most.

Row-indexed decoder input.  R = B M S rows; row r belongs to group r // S and scene (r // S) // M.  Forward without dropout:
row 0 = src[b,k] + memory[b,k], zeros for prop < 0; row 1 + t = emb[tok[r,1+t]] * float32(sqrt(D)) + pe[t]; mask[r,q,k] =
tok[r,k] > 0 and k <= q.  Backward: d_rows[b,k] = sum of g[r,0] over the scene's groups with prop == k, group then sample
ascending, from float32 0, every addition rounded."""
import collections
import functools

import numpy as np

import self_critical_restated as SC

F32, F64 = np.float32, np.float64

Selection = collections.namedtuple("Selection", "prop obj slot_of key dist n_sel")


def near2_of(near):
    return F32(F32(near) * F32(near))


def distances(xyz_b, centre):
    """d over the K proposals of one scene for one object centre, float32, in the kernel's order"""
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (xyz_b[:, i].astype(F32) - F32(centre[i]) for i in range(3))
        return ((dx * dx).astype(F32) + (dz * dz).astype(F32)).astype(F32) + (dy * dy).astype(F32)


def nearest(xyz_b, centre):
    """(k, d) of the first minimum, NaN never one; (-1, inf) without a finite minimum"""
    best, bk = F32(np.inf), -1
    for k, d in enumerate(distances(xyz_b, centre)):
        if d < best:
            best, bk = d, k
    return bk, best


def candidates(xyz, center, label_mask, object_ids, dataset_idx, key_table, nkeys, near):
    """per scene the list of (d, j, k, key row) of the qualifying objects, in slot order"""
    n2 = near2_of(near)
    B, G = label_mask.shape
    out = []
    for b in range(B):
        rows = []
        for j in range(G):
            if not label_mask[b, j] > 0:
                continue
            key = SC.key_row(np.reshape(dataset_idx, -1)[b], object_ids[b, j], key_table, nkeys)
            if key < 0:
                continue
            k, d = nearest(xyz[b], center[b, j])
            if k >= 0 and d < n2:
                rows.append((d, j, k, key))
        out.append(rows)
    return out


def _fill(per_scene, object_ids, M):
    B = len(per_scene)
    s = Selection(np.full((B, M), -1, np.int64), np.full((B, M), -1, np.int64), np.full((B, M), -1, np.int32),
                  np.full((B, M), -1, np.int32), np.full((B, M), np.inf, F32), np.zeros(B, np.int32))
    for b, rows in enumerate(per_scene):
        for m, (d, j, k, key) in enumerate(rows[:M]):
            s.prop[b, m], s.obj[b, m], s.slot_of[b, m], s.key[b, m], s.dist[b, m] = k, object_ids[b, j], j, key, d
        s.n_sel[b] = min(len(rows), M)
    return s


def select(xyz, center, label_mask, object_ids, dataset_idx, key_table, nkeys, near, M):
    """what spacap_scst_select_f32 writes: the rank of an object is the number of qualifying objects in front of it"""
    per_scene = []
    for rows in candidates(xyz, center, label_mask, object_ids, dataset_idx, key_table, nkeys, near):
        ranked = [None] * len(rows)
        for d, j, k, key in rows:
            rank = sum(1 for d2, j2, _, _ in rows if d2 < d or (d2 == d and j2 < j))
            ranked[rank] = (d, j, k, key)
        per_scene.append(ranked)
    return _fill(per_scene, object_ids, M)


def select_brute(xyz, center, label_mask, object_ids, dataset_idx, key_table, nkeys, near, M):
    """the same by another road: float64 arg-min over the float32 distances, ``sorted`` on (d, j) tuples"""
    n2 = float(near2_of(near))
    B, G = label_mask.shape
    per_scene = []
    for b in range(B):
        rows = []
        for j in range(G):
            key = SC.key_row(np.reshape(dataset_idx, -1)[b], object_ids[b, j], key_table, nkeys)
            d = distances(xyz[b], center[b, j]).astype(F64)
            if label_mask[b, j] <= 0 or key < 0 or np.isnan(d).all():
                continue
            k = int(np.nanargmin(d))
            if np.isfinite(d[k]) and d[k] < n2:
                rows.append((float(d[k]), j, k, key))
        per_scene.append(sorted(rows, key=lambda r: (r[0], r[1])))
    return _fill(per_scene, object_ids, M)


# ---- the selection cases of both test modules ------------------------------------------------------------------------------
SELECT_CASES = ((1, 1, 1, 1), (2, 31, 5, 5), (3, 64, 128, 16), (2, 65, 128, 128), (2, 256, 128, 16), (1, 257, 256, 3))
SELECT_NEAR = 0.75            # near2 = 0.5625: both exact in float32
SELECT_NKEYS = 7
SelectInputs = collections.namedtuple("SelectInputs", "xyz center label_mask object_ids dataset_idx key_table")
FEATURES = ("two proposals at the same distance", "two objects with bit-equal d", "d equal to near2 is excluded",
            "the float32 below near2 is included", "a masked slot", "an id behind a -1 entry", "a negative id", "an id too large",
            "a dataset_idx outside the table", "a NaN centre", "a scene with no qualifying object", "more than M qualify",
            "fewer than M qualify", "two objects share a proposal")


@functools.lru_cache(maxsize=None)
def select_inputs(case):
    """Proposals on a unit lattice (exact squares), scenes by role: b % 3 == 0 carries the constructed slots -- the midpoint of
    two proposals, d == near2 and the float32 below it off the lattice's corner, a masked slot, the ids without a key row, a NaN
    centre --, b % 3 == 1 an object in every slot (off-lattice random offsets, and two slots at the same exact offset), b % 3 == 2
    a dataset_idx outside the table."""
    B, K, G, M = case
    rng = np.random.default_rng(4000 + 7 * K + G)
    k = np.arange(K)
    lattice = np.stack([k % 8, (k // 8) % 8, k // 64], 1).astype(F32)
    xyz = np.repeat(lattice[None], B, 0).copy()
    center = np.zeros((B, G, 3), F32)
    mask = np.zeros((B, G), F32)
    ids = np.repeat((G - 1 - np.arange(G))[None], B, 0).astype(np.int64)          # slot j carries id G - 1 - j
    didx = np.arange(B, dtype=np.int64)
    table = np.full((B, G + 2), -1, np.int32)
    table[:, :G] = (np.arange(B)[:, None] * G + np.arange(G)[None]) % SELECT_NKEYS
    table[:, G + 1] = SELECT_NKEYS                                                   # an entry behind the last key row
    below = F32(np.nextafter(F32(SELECT_NEAR), F32(0)))
    for b in range(B):
        if b % 3 == 0:
            slots = [((0.5, 0, 0), 1, None), ((-SELECT_NEAR, 0, 0), 1, None), ((-below, 0, 0), 1, None), ((0.25, 0, 0), 0, None),
                     ((0, 0.25, 0), 1, G), ((0, 0, 0.25), 1, -1), ((0, 0, -0.25), 1, G + 2), ((0, np.nan, 0), 1, None),
                     ((0.25, 0.25, 0), 1, G + 1)]
            for j, (c, m, oid) in enumerate(slots[:G]):
                center[b, j], mask[b, j] = c, m
                if oid is not None:
                    ids[b, j] = oid
        elif b % 3 == 1:
            for j in range(G):
                kj = (7 * j + 3) % K
                off = rng.uniform(-0.3, 0.3, 3).astype(F32) if j % 2 else rng.integers(-16, 17, 3).astype(F32) / F32(64)
                if j < 2:
                    off = np.array([0.25, 0, 0], F32)
                center[b, j], mask[b, j] = xyz[b, kj] + off, 1
                if j % 9 == 8:
                    mask[b, j] = 0
                if j % 11 == 10:
                    ids[b, j] = G
        else:
            center[b], mask[b] = xyz[b, np.arange(G) % K], 1
            didx[b] = B + 1
    out = SelectInputs(xyz, center, mask, ids, didx, table)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def select_reference(case):
    x = select_inputs(case)
    return select(x.xyz, x.center, x.label_mask, x.object_ids, x.dataset_idx, x.key_table, SELECT_NKEYS, SELECT_NEAR, case[3])


def select_features(case):
    """which of FEATURES the inputs of ``case`` contain, read off the restatement"""
    B, K, G, M = case
    x, ref = select_inputs(case), select_reference(case)
    n2 = near2_of(SELECT_NEAR)
    found = set()
    rows = candidates(x.xyz, x.center, x.label_mask, x.object_ids, x.dataset_idx, x.key_table, SELECT_NKEYS, SELECT_NEAR)
    for b in range(B):
        q = rows[b]
        inside = 0 <= x.dataset_idx[b] < x.key_table.shape[0]
        if not inside:
            found.add("a dataset_idx outside the table")
        if not q:
            found.add("a scene with no qualifying object")
        found.add("more than M qualify" if len(q) > M else "fewer than M qualify" if len(q) < M else "")
        taken = [int(p) for p in ref.prop[b] if p >= 0]
        if len(set(taken)) < len(taken):
            found.add("two objects share a proposal")
        sel_d = ref.dist[b][:ref.n_sel[b]]
        if (sel_d[1:] == sel_d[:-1]).any():
            found.add("two objects with bit-equal d")
            i = int(np.flatnonzero(sel_d[1:] == sel_d[:-1])[0])
            assert ref.slot_of[b, i] < ref.slot_of[b, i + 1]
        if (sel_d == np.nextafter(n2, F32(0))).any():
            found.add("the float32 below near2 is included")
        for j in range(G):
            if not x.label_mask[b, j] > 0:
                found.add("a masked slot")
                continue
            oid = int(x.object_ids[b, j])
            if inside and oid < 0:
                found.add("a negative id")
            elif inside and oid >= x.key_table.shape[1]:
                found.add("an id too large")
            elif inside and x.key_table[b, oid] == -1:
                found.add("an id behind a -1 entry")
            if np.isnan(x.center[b, j]).any():
                found.add("a NaN centre")
                assert j not in ref.slot_of[b]
            if not inside or SC.key_row(x.dataset_idx[b], oid, x.key_table, SELECT_NKEYS) < 0:
                continue
            d = distances(x.xyz[b], x.center[b, j])
            if np.isnan(d).all():
                continue
            if (d == np.nanmin(d)).sum() >= 2 and np.nanmin(d) < n2:
                found.add("two proposals at the same distance")
                assert j in ref.slot_of[b][:ref.n_sel[b]] or len(q) > M
                if j in ref.slot_of[b]:
                    assert ref.prop[b][list(ref.slot_of[b]).index(j)] == int(np.flatnonzero(d == np.nanmin(d))[0])
            if np.nanmin(d) == n2:
                found.add("d equal to near2 is excluded")
                assert j not in ref.slot_of[b]
    found.discard("")
    return found


# ---- the row-indexed decoder input -----------------------------------------------------------------------------------------
def pe_table(n, D):
    """the sinusoid rows of PositionalEncoding, float32 (tests pass the module's own table to the kernels; this one feeds the
    CPU checks)"""
    pos = np.arange(n, dtype=F64)[:, None]
    div = np.exp(np.arange(0, D, 2, dtype=F64) * -(np.log(10000.0) / D))
    pe = np.zeros((n, D), F64)
    pe[:, 0::2] = np.sin(pos * div)
    pe[:, 1::2] = np.cos(pos * div)[:, :D // 2]
    return pe.astype(F32)


def prep_rows_fwd(src, memory, prop, tok, emb, pe, M, S):
    """(x0 (R, L, D) float32, mask (R, L, L) uint8) without dropout"""
    B, K, D = src.shape
    R, T = tok.shape
    L, V = T - 1, emb.shape[0]
    prop = np.reshape(prop, -1)
    sqrt_d = F32(np.sqrt(F64(D)))
    x0 = np.zeros((R, L, D), F32)
    mask = np.zeros((R, L, L), np.uint8)
    for r in range(R):
        g = r // S
        b, k = g // M, int(prop[g])
        if 0 <= k < K:
            x0[r, 0] = src[b, k] + memory[b, k] if memory is not None else src[b, k]
        for row in range(1, L):
            t = min(max(int(tok[r, row]), 0), V - 1)
            x0[r, row] = (emb[t] * sqrt_d).astype(F32) + pe[row - 1]
        live = tok[r, :L] > 0
        mask[r] = np.tril(np.ones((L, L), bool)) & live[None, :]
    return x0, mask


def prep_rows_bwd(g, prop, B, K, M, S):
    """d_rows (B, K, D) float32: sequential float32 sums in (group, sample) order; and per element the number of rows added"""
    R, L, D = g.shape
    prop = np.reshape(prop, -1)
    d = np.zeros((B, K, D), F32)
    n = np.zeros((B, K), np.int64)
    for grp in range(B * M):
        k = int(prop[grp])
        if not 0 <= k < K:
            continue
        b = grp // M
        for s in range(S):
            d[b, k] = d[b, k] + g[grp * S + s, 0]
            n[b, k] += 1
    return d, n


PREP_CASES = ((1, 1, 1, 1, 64, 2, 5), (2, 32, 3, 2, 128, 3, 300), (2, 256, 4, 3, 128, 33, 300), (3, 7, 2, 5, 200, 33, 120))
PrepInputs = collections.namedtuple("PrepInputs", "xyz src memory prop tok emb g")


@functools.lru_cache(maxsize=None)
def prep_inputs(case):
    """(B,K,M,S,D,T,V): distinct proposal points; the first two or three groups of scene 0 hold ONE proposal (where M > 1), one
    group of another scene (of scene 0 where B = 2) is empty, the last scene of B > 1 is empty altogether; token rows end in
    padding and two ids lie outside the table."""
    B, K, M, S, D, T, V = case
    rng = np.random.default_rng(5000 + 3 * K + D + T)
    xyz = (rng.permutation(4 * K)[:K, None] + rng.uniform(0.0, 0.25, (B, K, 3))).astype(F32)      # distinct by construction
    src, memory = rng.normal(0, 1, (B, K, D)).astype(F32), rng.normal(0, 1, (B, K, D)).astype(F32)
    prop = rng.integers(0, K, (B, M)).astype(np.int64)
    prop[0, :min(M, 3)] = K // 2
    if B > 2:
        prop[1, M - 1] = -1
    elif M > 2:
        prop[0, M - 1] = -1
    if B > 1:
        prop[B - 1, :] = -1
    R = B * M * S
    tok = rng.integers(1, V, (R, T)).astype(np.int64)
    for r in range(R):
        if T > 2:
            tok[r, rng.integers(2, T):] = 0
    if R > 2 and T > 2:
        tok[1, 1], tok[2, 1] = V + 3, -2                                  # clamped into the table, as the kernel does
    emb = rng.normal(0, 1, (V, D)).astype(F32)
    g = rng.normal(0, 1, (R, T - 1, D)).astype(F32)
    out = PrepInputs(xyz, src, memory, prop, tok, emb, g)
    for a in out:
        a.setflags(write=False)
    return out
