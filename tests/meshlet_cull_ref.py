"""NumPy fp32 restatement of the reference's meshlet_cull.comp with inc/meshlet_render.h: every step one IEEE fp32 operation in the
shader's order (dot sums left to right, matrix x vector column by column, vector x matrix one dot per column, normalize = a / sqrt(dot)).
tests/golden/make_meshlet_cull_golden.py asserts it equal to the executed shader on every stored case; GPU tests use it for scenes
beyond the stored ones.

A scene is a dict of arrays:
    tasks (T, 5) uint32      {aabb_instance, occluder_state_offset, node_instance, mesh_index_count, material_flags}
    aabbs (A, 8) float32     {lo.xyz, pad, hi.xyz, pad}
    transforms (N, 12) float32   three rows of four
    bounds (B, 8) float32    {centre.xyz, radius, cone.xyz, cutoff};  draws (B, 3) uint32 {index_count, first_index, vertex_offset}
    occluders (O,) uint32;   output (D,) uint32 as it is before the launch (count words zero)
    frustum (56,) uint32     the 224-byte block;  camera (3,) float32
    chain (n,) float32 with chain_width, chain_height, chain_levels (phase 2)
cull() returns (output, occluders, info) after one dispatch; the records of one task are contiguous and in lane order, tasks in the order
the shader's groups run one after the other.  An index outside its array makes the element not visible, as the kernel has it (the
shader has no such rule; the stored cases have no such index).  info counts what decided, for the generator's coverage assertions."""
import numpy as np

F = np.float32
ORTHO, SKINNED, FORCE_VISIBLE = 1, 2, 4
POISON = 0xCD
POISON_WORD = 0xCDCDCDCD


def frustum_fields(frustum):
    u = np.ascontiguousarray(frustum, np.uint32)
    assert u.shape == (56,)
    f, i = u.view(np.float32), u.view(np.int32)
    return {"viewport": f[0:4], "planes": f[4:28].reshape(6, 4), "view": f[28:44].reshape(4, 4), "scale_bias": f[44:48],
            "hiz_resolution": i[48:50], "winding": f[50], "hiz_min_lod": int(i[51]), "hiz_max_lod": int(i[52])}


def pack_frustum(planes, view_columns, scale_bias=(0, 0, 0, 0), viewport=(0, 0, 0, 0), hiz_resolution=(0, 0), winding=1.0, hiz_min_lod=0, hiz_max_lod=0):
    u = np.zeros(56, np.uint32)
    f, i = u.view(np.float32), u.view(np.int32)
    f[0:4] = viewport
    f[4:28] = np.asarray(planes, np.float32).reshape(24)
    f[28:44] = np.asarray(view_columns, np.float32).reshape(16)
    f[44:48] = scale_bias
    i[48:50] = hiz_resolution
    f[50] = winding
    i[51], i[52] = hiz_min_lod, hiz_max_lod
    return u


def level_sizes(width, height, levels):
    return [(max(width >> l, 1), max(height >> l, 1)) for l in range(levels)]


def dot_point(v, p):
    return v[:, 0] * p[0] + v[:, 1] * p[1] + v[:, 2] * p[2] + p[3]


def dot3(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def find_msb(v):
    """GLSL findMSB(int): -1 for 0 and -1, the highest 0 bit of a negative value."""
    u = np.where(v < 0, ~v, v).astype(np.int64)
    r = np.full(v.shape, -1, np.int32)
    for b in range(32):
        r = np.where((u >> b) != 0, b, r)
    return r.astype(np.int32)


def to_int(x):
    with np.errstate(invalid="ignore"):
        c = np.where(np.isnan(x), F(-2147483648.0), np.minimum(np.maximum(x, F(-2147483648.0)), F(2147483520.0)))
    return c.astype(np.int64).astype(np.int32)  # truncation toward zero


def glsl_clamp(v, lo, hi):
    return np.minimum(np.maximum(v, lo), hi)


def hiz_cull(scene, fr, lo_x, hi_x, lo_y, hi_y, closest_z, info):
    sb, res = fr["scale_bias"], fr["hiz_resolution"]
    ix0, ix1 = to_int(lo_x * sb[0] + sb[2]), to_int(hi_x * sb[0] + sb[2])
    iy0, iy1 = to_int(lo_y * sb[1] + sb[3]), to_int(hi_y * sb[1] + sb[3])
    info["span_left"] += int((ix0 < 0).sum())
    info["span_right"] += int((ix1 > res[0] - 1).sum())
    info["span_top"] += int((iy0 < 0).sum())
    info["span_bottom"] += int((iy1 > res[1] - 1).sum())
    ix0 = glsl_clamp(ix0, 0, res[0] - 1)
    ix1 = glsl_clamp(ix1, ix0, res[0] - 1)
    iy0 = glsl_clamp(iy0, 0, res[1] - 1)
    iy1 = glsl_clamp(iy1, iy0, res[1] - 1)
    max_delta = np.maximum(ix1 - ix0, iy1 - iy0)
    raw = find_msb(max_delta - 1) + 1
    lod = glsl_clamp(raw, fr["hiz_min_lod"], fr["hiz_max_lod"]).astype(np.int32)
    for d in (0, 1, 2, 3):
        info[f"delta_{d}"] += int((max_delta == d).sum())
    info["delta_many"] += int((max_delta > 3).sum())
    info["lod_at_min"] += int((raw < fr["hiz_min_lod"]).sum())
    info["lod_at_max"] += int((raw > fr["hiz_max_lod"]).sum())
    info["lod_between"] += int(((raw > fr["hiz_min_lod"]) & (raw < fr["hiz_max_lod"])).sum())
    mx = np.maximum(res[0] >> lod, 1) - 1
    my = np.maximum(res[1] >> lod, 1) - 1
    ix0, ix1 = np.minimum(ix0 >> lod, mx), np.minimum(ix1 >> lod, mx)
    iy0, iy1 = np.minimum(iy0 >> lod, my), np.minimum(iy1 >> lod, my)
    level = lod - fr["hiz_min_lod"]
    sizes = level_sizes(scene["chain_width"], scene["chain_height"], scene["chain_levels"])
    offsets = np.concatenate([[0], np.cumsum([w * h for w, h in sizes])]).astype(np.int64)
    widths, heights = np.array([w for w, _ in sizes], np.int64), np.array([h for _, h in sizes], np.int64)
    assert level.size == 0 or (level.min() >= 0 and level.max() < len(sizes)), "the frustum block does not describe the chain"
    chain = np.asarray(scene["chain"], np.float32)

    def texel(x, y):
        x = np.minimum(np.maximum(x, 0), widths[level] - 1)
        y = np.minimum(np.maximum(y, 0), heights[level] - 1)
        return chain[offsets[level] + y * widths[level] + x]

    nx, ny = ix1 != ix0, iy1 != iy0
    info["taps_1"] += int((~nx & ~ny).sum())
    info["taps_2x"] += int((nx & ~ny).sum())
    info["taps_2y"] += int((~nx & ny).sum())
    info["taps_4"] += int((nx & ny).sum())
    d = texel(ix0, iy0)
    d = np.where(nx, np.maximum(d, texel(ix0 + 1, iy0)), d)
    d = np.where(ny, np.maximum(d, texel(ix0, iy0 + 1)), d)
    d = np.where(nx & ny, np.maximum(d, texel(ix0 + 1, iy0 + 1)), d)
    return closest_z < d


def project_sphere_flat(xy, z, r):
    length = np.sqrt(xy * xy + z * z)
    s = r / length
    c = np.sqrt(F(1.0) - s * s)
    lo_x, lo_y = c * xy + (-s) * z, s * xy + c * z
    hi_x, hi_y = c * xy + s * z, (-s) * xy + c * z
    return lo_x / lo_y, hi_x / hi_y


def cluster_cull_hiz(scene, fr, flags, center, radius, info, who):
    """center (N, 3), radius (N,): visible (N,) bool"""
    view = fr["view"]
    v = [view[0, i] * center[:, 0] + view[1, i] * center[:, 1] + view[2, i] * center[:, 2] + view[3, i] for i in range(3)]
    vx, vy, vz = v[0], -v[1], -v[2]
    ortho = bool(flags & ORTHO)
    test = np.ones(len(radius), bool) if ortho else vz > radius + F(0.1)
    ret = np.ones(len(radius), bool)
    info[who + "_near_accept"] += int((~test).sum())
    if test.any():
        x, y, z, r = vx[test], vy[test], vz[test], radius[test]
        if ortho:
            x0, x1, y0, y1 = x + (-r), x + r, y + (-r), y + r
        else:
            x0, x1 = project_sphere_flat(x, z, r)
            y0, y1 = project_sphere_flat(y, z, r)
        got = hiz_cull(scene, fr, x0, x1, y0, y1, z - r, info)
        info[who + "_hiz_reject"] += int((~got).sum())
        info[who + "_hiz_accept"] += int(got.sum())
        ret[test] = got
    return ret


def cluster_cull(scene, fr, phase, flags, m, b, info):
    """m (N, 12), b (N, 8): visible (N,) bool"""
    rows = m.reshape(-1, 3, 4)
    c = b[:, 0:3]
    center = np.stack([c[:, 0] * rows[:, i, 0] + c[:, 1] * rows[:, i, 1] + c[:, 2] * rows[:, i, 2] + rows[:, i, 3] for i in range(3)], 1)
    s = [rows[:, 0, j] * rows[:, 0, j] + rows[:, 1, j] * rows[:, 1, j] + rows[:, 2, j] * rows[:, 2, j] for j in range(3)]
    radius = b[:, 3] * np.sqrt(np.maximum(np.maximum(s[0], s[1]), s[2]))
    cone = b[:, 4:8]
    t = np.stack([cone[:, 0] * rows[:, i, 0] + cone[:, 1] * rows[:, i, 1] + cone[:, 2] * rows[:, i, 2] for i in range(3)], 1)
    n = t / np.sqrt(dot3(t, t))[:, None]
    d = center - np.asarray(scene["camera"], np.float32)[None, :]
    has_cone = cone[:, 3] < F(1.0)
    cone_ok = ~has_cone | (dot3(d, n) <= cone[:, 3] * np.sqrt(dot3(d, d)) + radius)
    info["chunk_no_cone"] += int((~has_cone).sum())
    info["chunk_cone_reject"] += int((~cone_ok).sum())
    info["chunk_cone_accept"] += int((has_cone & cone_ok).sum())
    ret = cone_ok.copy()
    for i in range(6):
        out = dot_point(center, fr["planes"][i]) < -radius
        info[f"chunk_plane_{i}_reject"] += int((ret & out).sum())
        ret &= ~out
    if phase == 2 and ret.any():
        ret[ret] = cluster_cull_hiz(scene, fr, flags, center[ret], radius[ret], info, "chunk")
    return ret


def frustum_cull(scene, fr, phase, flags, boxes, info):
    lo, hi = boxes[:, 0:3], boxes[:, 4:7]
    ret = np.ones(len(boxes), bool)
    for i in range(6):
        p = fr["planes"][i]
        m = np.where((p[0:3] > F(0.0))[None, :], hi, lo)
        out = dot_point(m, p) < F(0.0)
        info[f"aabb_plane_{i}_reject"] += int((ret & out).sum())
        ret &= ~out
    if phase == 2 and ret.any():
        e = hi[ret] - lo[ret]
        ret[ret] = cluster_cull_hiz(scene, fr, flags, F(0.5) * (lo[ret] + hi[ret]), F(0.5) * np.sqrt(dot3(e, e)), info, "aabb")
    return ret


class Info(dict):
    def __missing__(self, key):
        return 0


def cull(scene, phase, flags, offset, count, mdi_count_offset, draw_indirect_offset):
    """One dispatch.  Returns (output, occluders, info)."""
    fr = frustum_fields(scene["frustum"])
    info = Info()
    tasks = np.asarray(scene["tasks"], np.uint32).reshape(-1, 5)
    aabbs = np.asarray(scene["aabbs"], np.float32).reshape(-1, 8)
    transforms = np.asarray(scene["transforms"], np.float32).reshape(-1, 12)
    bounds = np.asarray(scene["bounds"], np.float32).reshape(-1, 8)
    draws = np.asarray(scene["draws"], np.uint32).reshape(-1, 3)
    occluders = np.array(scene["occluders"], np.uint32)
    output = np.array(scene["output"], np.uint32)
    skinned = bool(flags & SKINNED)

    def occluder(i):
        return int(occluders[i]) if i < len(occluders) else 0

    with np.errstate(all="ignore"):
        index = np.arange(offset, offset + count, dtype=np.int64)
        index = index[index < len(tasks)]
        mine = tasks[index]
        ok = mine[:, 0] < len(aabbs)
        visible = np.zeros(len(mine), bool)
        visible[ok] = frustum_cull(scene, fr, phase, flags, aabbs[mine[ok, 0]], info)
        info["aabb_accept"] += int(visible.sum())
        work = []
        for k, t in enumerate(mine):
            needs = bool(visible[k])
            if phase == 1:
                needs = needs and occluder(t[1]) != 0
                info["task_word_zero"] += int(visible[k] and not needs)
            elif phase == 2 and not needs and t[1] < len(occluders):
                occluders[t[1]] = 0
                info["task_word_cleared"] += 1
            if needs:
                work.append(k)
        # every (task, lane) candidate at once
        pairs = []
        for k in work:
            t = mine[k]
            first, n, old = int(t[3]) & ~31, (int(t[3]) & 31) + 1, occluder(t[1])
            for lane in range(n):
                chunk = first + lane
                if chunk >= len(draws):
                    continue
                if phase == 1 and not (old >> lane) & 1:
                    info["chunk_bit_clear"] += 1
                    continue
                if not skinned and (chunk >= len(bounds) or t[2] >= len(transforms)):
                    continue
                pairs.append((k, lane, chunk, int(t[2])))
        info["tasks_processed"] += len(work)
        info["chunk_candidates"] += len(pairs)
        alive = np.ones(len(pairs), bool)
        if pairs and not skinned:
            p = np.array(pairs, np.int64)
            alive = cluster_cull(scene, fr, phase, flags, transforms[p[:, 3]], bounds[p[:, 2]], info)
        info["chunk_accept"] += int(alive.sum())
        by_task = {}
        for (k, lane, chunk, _), a in zip(pairs, alive):
            if a:
                by_task.setdefault(k, []).append((lane, chunk))
        for k in work:
            t = mine[k]
            lanes = by_task.get(k, [])
            if phase == 2:
                old = occluder(t[1])
                if t[1] < len(occluders):
                    occluders[t[1]] = sum(1 << lane for lane, _ in lanes)
                if not flags & FORCE_VISIBLE:
                    info["chunk_drawn_in_phase_1"] += sum(1 for lane, _ in lanes if (old >> lane) & 1)
                    lanes = [(lane, chunk) for lane, chunk in lanes if not (old >> lane) & 1]
            if not lanes:
                continue
            base = int(output[mdi_count_offset])
            output[mdi_count_offset] = np.uint32((base + len(lanes)) & 0xFFFFFFFF)
            for j, (lane, chunk) in enumerate(lanes):
                at = draw_indirect_offset + 5 * (base + j)
                if at + 5 <= len(output):
                    output[at:at + 5] = (draws[chunk, 0], 1, draws[chunk, 1], draws[chunk, 2], index[k])
            info["draws"] += len(lanes)
    return output, occluders, info


def records(output, mdi_count_offset, draw_indirect_offset):
    """(count, (n, 5) records in buffer order), n = the records that fit"""
    count = int(output[mdi_count_offset])
    fit = max(min(count, (len(output) - draw_indirect_offset) // 5), 0)
    return count, output[draw_indirect_offset:draw_indirect_offset + 5 * fit].reshape(fit, 5)


def sorted_records(r):
    """sorted by (task_index, first_index)"""
    return r[np.lexsort((r[:, 2], r[:, 4]))] if len(r) else r


def assert_task_order(r, draws, tasks):
    """Each task's records are contiguous and in lane order (its chunks' first_index in the order of the chunks)."""
    seen, at = set(), 0
    draws = np.asarray(draws, np.uint32).reshape(-1, 3)
    while at < len(r):
        task = int(r[at, 4])
        assert task not in seen, f"task {task}'s records are not contiguous"
        seen.add(task)
        end = at
        while end < len(r) and int(r[end, 4]) == task:
            end += 1
        first = int(tasks[task][3]) & ~31
        lanes = []
        for rec in r[at:end]:
            match = [l for l in range(32) if first + l < len(draws) and np.array_equal(draws[first + l], rec[[0, 2, 3]])]
            assert match, f"task {task}: a record is no chunk of the task"
            lanes.append(match[0])
        assert lanes == sorted(lanes) and len(set(lanes)) == len(lanes), f"task {task}: records not in lane order {lanes}"
        at = end
