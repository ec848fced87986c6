"""CPU: the bloom sweep's case lists (tests/post_sweep.py) cover what they claim, and no case in them asks a kernel to stage more than its LDS
patch holds.  Plain Python over the level sizes; the kernel library is only asked its context-free gr_bloom_*_supported queries, last."""
import collections
import itertools

import numpy as np

import post_sweep as ps

MID, TAIL = ("threshold", "d0", "d1"), ("d1", "d2", "d3")


def parity_levels():
    return [ps.frame_levels(w, h) for w, h in ps.PARITY_SWEEP]


def test_parity_sweep_reaches_every_template_combination():
    """From the level sizes alone: which instantiation each launch gets over the parity sweep (frames the committed rules offer the launch for).

    k_bloom_down_pair<A_EXACT, B_EXACT> as gr_bloom_down_mid and as gr_bloom_down_tail: all four combinations each.
    k_bloom_up_tail<U2_EXACT, U1_EXACT>: all four.
    k_bloom_up_all<U2_EXACT, U1_EXACT> (upsample-0 exactly twice upsample-1: the quarter level even): all four.
    k_bloom_pyramid<D2_EXACT, D3_EXACT, U2_EXACT, U1_EXACT>: 4 of the 16 on frames, 8 with the off-pyramid levels.  Cannot occur:
      * U2_EXACT != D3_EXACT (8 combinations), anywhere: the launcher requires upsample-2 to have downsample-2's size (pyramid_own_fits), and both
        flags compare that size with downsample-3's;
      * U1_EXACT != D2_EXACT (4 more) on a frame: upsample-1 has downsample-1's size there and both flags compare it with the sixteenth level's.  The
        launcher itself takes an upsample-1 of another size: ps.pyramid_offpyramid_cases() reaches those four.
    DYNAMIC_EXPOSURE / LUMINANCE / FEEDBACK and the HDR format do not depend on the size: the GPU test crosses them with every frame of the sweep."""
    levels = parity_levels()
    both = set(itertools.product((False, True), repeat=2))
    assert {ps.mid_flags(l) for l in levels if ps.mid_offered(l)} == both
    assert {ps.down_tail_flags(l) for l in levels if ps.tail_offered(l)} == both
    assert {ps.up_flags(l) for l in levels if ps.tail_offered(l)} == both
    assert {ps.up_flags(l) for l in levels if ps.up_all_offered(l)} == both
    on_frames = {ps.pyramid_flags(l) for l in levels if ps.pyramid_offered(l)}
    assert on_frames == {(d2, d3, d3, d2) for d2, d3 in both}
    off = {ps.pyramid_flags(l) for l in ps.pyramid_offpyramid_cases()}
    assert all(ps.pyramid_fits(l) for l in ps.pyramid_offpyramid_cases())
    assert off == {(d2, d3, d3, not d2) for d2, d3 in both}
    assert len(on_frames | off) == 8
    # the head has no size flag; it must be offered on part of the sweep and declined on part of it
    assert {ps.head_offered(l) for l in levels} == {False, True}
    # every level down to downsample-3 takes both the exact half and the ceil, in each dimension
    for fine, coarse in (("hdr", "threshold"), ("threshold", "d0"), ("d0", "d1"), ("d1", "d2"), ("d2", "d3")):
        for axis in (0, 1):
            assert {l[fine][axis] == 2 * l[coarse][axis] for l in levels} == {False, True}, (fine, coarse, axis)
    assert min(min(l["d3"]) for l in levels) >= 3


def test_every_remainder_of_the_last_tile_occurs():
    """Width and height of the tiled level modulo the tile, over everything the GPU test launches (parity sweep where the launch is offered + the
    level pairs).  8 x 8 tiles (downsample-1 of down_mid / down_head, downsample-3 of down_tail): every remainder 0 .. 7 -- but for the head,
    whose downsample-1 is an eighth of a frame the sweep makes 65 .. 160 wide: 9 .. 20, every remainder too.  32 x 32 tiles of upsample-1
    (up_tail): every remainder 0 .. 31.  32 x 32 tiles of upsample-0 (up_all): the level is twice upsample-1, so only the 16 even remainders can
    occur, and all of them do.  The pyramid runs the same up_all_block on 12 of them (the frames the query offers it are too few for the rest,
    which gr_bloom_up_all's cases cover in that block).  The sweep holds every frame and its transpose, so both axes see the same sets."""
    levels = parity_levels()
    mid = [l for l in levels if ps.mid_offered(l)] + [l for l, taken in ps.down_pair_cases(MID) if taken]
    tail_down = [l for l in levels if ps.tail_offered(l)] + [l for l, taken in ps.down_pair_cases(TAIL) if taken]
    tail_up = [l for l in levels if ps.tail_offered(l)] + [l for l, taken in ps.up_tail_cases() if taken]
    up_all = [l for l in levels if ps.up_all_offered(l)] + [l for l, taken in ps.up_all_cases() if taken]
    head = [l for l in levels if ps.head_offered(l)]
    for axis in (0, 1):
        assert {l["d1"][axis] % 8 for l in mid} == set(range(8))
        assert {l["d1"][axis] % 8 for l in head} == set(range(8))
        assert {l["d3"][axis] % 8 for l in tail_down} == set(range(8))
        assert {l["u1"][axis] % 32 for l in tail_up} == set(range(32))
        assert {l["u0"][axis] % 32 for l in up_all} == set(range(0, 32, 2))
        # the pyramid's upsample-0 is a quarter of a frame 72 .. 160 wide whose eighth is whole: 18 .. 40 in steps of 2, plus the level cases' 26 .. 40
        pyramid = [l for l in levels if ps.pyramid_offered(l)] + ps.pyramid_offpyramid_cases()
        assert {l["u0"][axis] % 32 for l in pyramid} == {18, 20, 22, 24, 26, 28, 30, 0, 2, 4, 6, 8}


def test_off_pyramid_pairs_sit_on_the_boundaries_of_their_rules():
    for fine, coarse in ps.DOWN_AXIS_TAKEN[:4]:
        assert fine == 23 * coarse // 10 and coarse in (10, 19, 20, 100)  # floor(2.3 x coarse)
        assert ps.down_patch_fits((fine, fine), (coarse, coarse)) and not ps.down_patch_fits((fine + 1, fine), (coarse, coarse))
    assert (43, 19) in ps.DOWN_AXIS_TAKEN
    assert {(f == 2 * c - 1, f == 2 * c, f == c) for f, c in ps.DOWN_AXIS_TAKEN[4:]} == {(True, False, False), (False, True, False), (False, False, True)}
    assert {(2 * c == f, 2 * c == f + 1) for f, c in ps.UP_AXIS_TAKEN} == {(True, False), (False, True)}
    for cases, fits, names in ((ps.down_pair_cases(MID), ps.mid_fits, MID), (ps.down_pair_cases(TAIL), ps.down_tail_fits, TAIL),
                               (ps.up_tail_cases(), ps.up_tail_fits, None), (ps.up_all_cases(), ps.up_all_fits, None)):
        assert {taken for _, taken in cases} == {False, True}
        for levels, taken in cases:
            assert fits(levels) == taken, levels
    # the two axes take different cases somewhere: one exact and the other not
    assert any((l["d2"][0] == 2 * l["d3"][0]) != (l["d2"][1] == 2 * l["d3"][1]) for l, taken in ps.down_pair_cases(TAIL) if taken)
    assert any((l["u1"][0] == 2 * l["u2"][0]) != (l["u1"][1] == 2 * l["u2"][1]) for l, taken in ps.up_tail_cases() if taken)


def test_every_case_fits_its_patch_and_some_fill_it():
    """The patch each workgroup of each launched case stages (post.hip down_pair_block, k_bloom_up_tail, up_all_block restated in ps.*_extent),
    against the constants.  Largest extents over the lists:
      TAIL_PATCH = 24: reached (43 -> 19 texels, the tile starting at 8; 230 -> 100 at 80): the rule fine <= 2.3 x coarse has no slack.
      UPALL_P1 = 20: reached by every upsample-0 with an interior 32-texel tile (32 / 2 + 4).
      UP_PATCH = 24: 22 at most.  fine <= 2 x coarse <= fine + 1 keeps the scale within [1/2, 1/2 + 1 / (2 fine)]; on the generic taps the 32
        outputs of a tile starting at 32 k reach from floor(16 k + 0.25 - 1.375) - 1 = 16 k - 3 to floor(16 k + 15.75 + 0.375) + 2 = 16 k + 18:
        22 texels, two of the three slack texels of tap_span never read.  20 on the 1:2 stencil (32 / 2 + 4).  The constant has two to spare.
      UPALL_P2 = 18: 16 at most, the same way under the 20 texels of upsample-1 (from 8 k - 3 to 8 k + 12); 14 on the stencil.  Two to spare.
    test_patches_hold_every_accepted_pair_up_to_700_texels shows that no accepted pair at all reaches further."""
    levels = parity_levels()
    down = [(l["d0"], l["d1"]) for l in levels if ps.mid_offered(l)] + [(l["d2"], l["d3"]) for l in levels if ps.tail_offered(l)]
    down += [(l[n[1]], l[n[2]]) for n in (MID, TAIL) for l, taken in ps.down_pair_cases(n) if taken]
    up = [(l["u1"], l["u2"]) for l in levels if ps.tail_offered(l)] + [(l["u1"], l["u2"]) for l, taken in ps.up_tail_cases() if taken]
    up_all = [l for l in levels if ps.up_all_offered(l)] + [l for l, taken in ps.up_all_cases() if taken] + ps.pyramid_offpyramid_cases()
    for function in ("down_mid", "tail", "up_all"):
        for w, h in ps.committed_ones(function):
            l = ps.frame_levels(w, h)
            if function == "down_mid":
                down.append((l["d0"], l["d1"]))
            elif function == "tail":
                down.append((l["d2"], l["d3"]))
                up.append((l["u1"], l["u2"]))
            else:
                up_all.append(l)
    down_extents = [ps.down_extent(f, c)[0] for f, c in down]
    up_extents = [ps.up_tail_extent(f, c) for f, c in up]
    all_extents = [ps.up_all_extents(l["u0"], l["u1"], l["u2"]) for l in up_all]
    assert max(down_extents) == ps.TAIL_PATCH
    assert ps.down_extent((43, 43), (19, 19)) == (24, ("y", 8))
    assert max(up_extents) == 22 <= ps.UP_PATCH
    assert max(p1 for p1, _ in all_extents) == ps.UPALL_P1
    assert max(p2 for _, p2 in all_extents) == 16 <= ps.UPALL_P2
    print(f"patch extents over {len(down)} down pairs, {len(up)} up pairs, {len(up_all)} up-all pyramids: TAIL_PATCH {max(down_extents)}/24 "
          f"({down_extents.count(24)} cases full), UP_PATCH {max(up_extents)}/24, UPALL_P1 {max(p for p, _ in all_extents)}/20, "
          f"UPALL_P2 {max(p for _, p in all_extents)}/18")


def test_patches_hold_every_accepted_pair_up_to_700_texels():
    """Per axis, every (fine, coarse) the rules accept with fine <= 700: the staged extent on the generic taps (and on the stencil where the ratio
    is exactly two) stays within the patch -- for the down pair with the 8-texel tile starting on any texel, as a row band of gr_bloom_down_mid
    may place it; the upsample launches take whole levels only.  An accepted pair that did not fit would be an out-of-bounds LDS write: found here, never launched."""
    worst_down = worst_up = worst_p2 = 0
    for coarse in range(1, 701):
        fine = np.arange(1, 701)
        fine = fine[fine.astype(np.float32) <= np.float32(2.3) * np.float32(coarse)]
        lo = np.arange(0, coarse)  # a tile may start on any row: gr_bloom_down_mid's row band sets the first one (tile_y0 = first row + 8 k)
        hi = np.minimum(lo + ps.TAIL_TILE, coarse) - 1
        p0, p1 = ps.tap_span(lo[None, :], hi[None, :], coarse, fine[:, None], 1.75)
        worst_down = max(worst_down, int((p1 - p0 + 1).max()))
        # the upsample rule: fine = 2 coarse or 2 coarse - 1
        for up_fine in (2 * coarse, 2 * coarse - 1):
            if not 1 <= up_fine <= 700:
                continue
            assert ps.up_patch_fits((up_fine, up_fine), (coarse, coarse))
            worst_up = max(worst_up, ps.up_axis_extent(up_fine, coarse, False), ps.up_axis_extent(up_fine, coarse, up_fine == 2 * coarse))
            for exact in ((False, True) if up_fine == 2 * coarse else (False,)):
                p1_extent, p2_extent = ps.up_all_axis_extents(2 * up_fine, up_fine, coarse, exact)
                assert p1_extent <= ps.UPALL_P1
                worst_p2 = max(worst_p2, p2_extent)
    # 2:1 stencil of the down pair: 2 x 8 + 4
    assert max(min(2 * (lo + 7) + 3, 2 * c - 1) - max(2 * lo - 2, 0) + 1 for c in range(1, 351) for lo in range(c)) == 20  # any tile start here too
    assert worst_down == ps.TAIL_PATCH
    assert worst_up == 22 <= ps.UP_PATCH
    assert worst_p2 == 16 <= ps.UPALL_P2


def test_committed_ones_are_there_and_the_restated_rules_reproduce_the_table():
    """The sizes of the committed table whose answer is 1 -- the frame loop takes that launch there -- per function: none of the lists is empty,
    the limit grid is in them, and the rules as tests/post_sweep.py states them give the committed answer for every un-varied frame."""
    gen = ps.golden_generator()
    ids = {name for name, _, _ in gen.cases()}
    frames, functions = ps.committed_answers()
    assert functions == gen.FUNCTIONS == tuple(ps.OFFERED)
    assert all("%dx%d %s" % (w, h, form) in ids for (w, h), forms in frames.items() for form in forms)
    grid = set(gen.LIMIT_GRID)
    counts = {}
    for function in functions:
        ones = ps.committed_ones(function)
        counts[function] = (len(ones), len(grid & set(ones)))
        assert ones and grid & set(ones), function
    print("committed 1s (all, on the limit grid):", counts)
    for (w, h), forms in frames.items():
        levels = ps.frame_levels(w, h)
        for form, answer in forms.items():
            for i, function in enumerate(functions):
                want = ps.OFFERED[function](levels)
                if function == "pyramid" and form.endswith(" lum") and min(levels["d3"]) < 2:
                    want = False  # no texel in the luminance grid (downsample-3 / 2)
                assert want == (answer[i] == "1"), (w, h, form, function)


def test_the_library_offers_what_the_restated_rules_say():
    """The gr_bloom_*_supported queries on the parity sweep and the level pairs, which the committed table does not hold.  For a pair that only
    names the levels of one launch the others are given sizes that fit (downsample-1 twice downsample-2, upsample-1 twice upsample-2)."""
    from granite_amd import capi
    lib = capi.load_library()
    gen = ps.golden_generator()
    for w, h in ps.PARITY_SWEEP:
        levels = ps.frame_levels(w, h)
        for b10 in (False, True):
            got = gen.answers(lib, gen.frame(w, h, b10), True)
            want = "".join("1" if ps.OFFERED[f](levels) else "0" for f in gen.FUNCTIONS)
            assert got == want, (w, h, b10, got, want)
    down, up = capi.downsample_push, capi.upsample_push
    for levels, taken in ps.down_pair_cases(MID):
        im = ps.fake_images(levels)
        assert lib.gr_bloom_down_mid_supported(im["threshold"], im["d0"], im["d1"], down(im["d0"], im["threshold"]), down(im["d1"], im["d0"])) == int(taken), levels
    for levels, taken in ps.down_pair_cases(TAIL):
        full = dict(levels, u2=levels["d2"], u1=(2 * levels["d2"][0], 2 * levels["d2"][1]))
        im = ps.fake_images(full)
        got = lib.gr_bloom_tail_supported(im["d1"], im["d2"], im["d3"], im["u2"], im["u1"], down(im["d2"], im["d1"]), down(im["d3"], im["d2"]),
                                          up(im["u2"], im["d3"]), up(im["u1"], im["u2"]))
        assert got == int(taken) == int(ps.tail_offered(full)), levels
    for levels, taken in ps.up_tail_cases():
        full = dict(levels, d2=levels["u2"], d1=(2 * levels["u2"][0], 2 * levels["u2"][1]))
        im = ps.fake_images(full)
        got = lib.gr_bloom_tail_supported(im["d1"], im["d2"], im["d3"], im["u2"], im["u1"], down(im["d2"], im["d1"]), down(im["d3"], im["d2"]),
                                          up(im["u2"], im["d3"]), up(im["u1"], im["u2"]))
        assert got == int(taken) == int(ps.tail_offered(full)), levels
    for levels, taken in ps.up_all_cases():
        im = ps.fake_images(levels)
        got = lib.gr_bloom_up_all_supported(im["d3"], im["u2"], im["u1"], im["u0"], up(im["u2"], im["d3"]), up(im["u1"], im["u2"]), up(im["u0"], im["u1"]))
        assert got == int(taken), levels
    for levels in ps.pyramid_offpyramid_cases():
        im = ps.fake_images(levels)
        args = capi.pyramid_args(im["hdr"], {n: im[n] for n in ps.SCALES}, im["history"], 0.25, 0x7000000000, 0.5)
        assert lib.gr_bloom_pyramid_supported(args) == 1, levels


def test_how_many_cases_the_gpu_tests_run_and_what_each_combination_gets():
    """The lists as tests/test_gpu_post_sweep.py parametrizes them: cases per entry point and list (pinned: a list that shrinks is seen here), and
    at least one launched case for every template combination and for a full patch, per entry point."""
    counts = {f: collections.Counter(origin for origin, _, _, _ in ps.frame_cases(f, ps.CROSS[f])) for f in ps.OFFERED}
    assert {f: (c["parity"], c["committed 1s"]) for f, c in counts.items()} == {
        "down_mid": (380, 344), "down_head": (92, 54), "tail": (760, 705), "up_all": (190, 223), "pyramid": (92, 22)}
    pairs = {"down_mid": ps.down_pair_cases(MID), "down_tail": ps.down_pair_cases(TAIL), "up_tail": ps.up_tail_cases(), "up_all": ps.up_all_cases()}
    assert {n: (sum(t for _, t in c), sum(not t for _, t in c)) for n, c in pairs.items()} == {
        "down_mid": (26, 8), "down_tail": (26, 8), "up_tail": (48, 8), "up_all": (32, 5)}
    assert len(ps.pyramid_offpyramid_cases()) == 8 and len(ps.PARITY_SWEEP) == 380
    both = set(itertools.product((False, True), repeat=2))

    def launched(function, pair_list):
        return [l for _, _, l, _ in ps.frame_cases(function, 1)] + [l for l, taken in pair_list if taken]

    per_flags = {"down_mid": collections.Counter(ps.mid_flags(l) for l in launched("down_mid", pairs["down_mid"])),
                 "down_tail": collections.Counter(ps.down_tail_flags(l) for l in launched("tail", pairs["down_tail"])),
                 "up_tail": collections.Counter(ps.up_flags(l) for l in launched("tail", pairs["up_tail"])),
                 "up_all": collections.Counter(ps.up_flags(l) for l in launched("up_all", pairs["up_all"]))}
    for name, counter in per_flags.items():
        assert set(counter) == both and min(counter.values()) >= 20, (name, counter)
    pyramid = collections.Counter(ps.pyramid_flags(l) for l in launched("pyramid", [(l, True) for l in ps.pyramid_offpyramid_cases()]))
    assert len(pyramid) == 8 and min(pyramid.values()) >= 2, pyramid
    # a full TAIL_PATCH in both launches of k_bloom_down_pair, a full UPALL_P1 in up_all and the pyramid
    assert sum(ps.down_extent(l["d0"], l["d1"])[0] == ps.TAIL_PATCH for l in launched("down_mid", pairs["down_mid"])) >= 4
    assert sum(ps.down_extent(l["d2"], l["d3"])[0] == ps.TAIL_PATCH for l in launched("tail", pairs["down_tail"])) >= 4
    assert sum(ps.up_all_extents(l["u0"], l["u1"], l["u2"])[0] == ps.UPALL_P1 for l in launched("up_all", pairs["up_all"])) >= 100
    assert any(ps.up_all_extents(l["u0"], l["u1"], l["u2"])[0] == ps.UPALL_P1 for l in launched("pyramid", []))
    print({n: {"".join("01"[v] for v in k): c for k, c in sorted(counter.items())} for n, counter in list(per_flags.items()) + [("pyramid", pyramid)]})
