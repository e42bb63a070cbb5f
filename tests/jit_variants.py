"""The compile-time switches of the specialised kernel: a table and nothing else.

One entry per `WO_*` macro that sits under `#ifndef` in wo_device_common.h, the library
kernels' headers (wo_tracers.h, path_kernels.h, query_kernels.h) or the text scene_jit.c emits, and one per environment knob that rewrites that text.  Classes:

  variant          set through WOLOLO_JIT_FLAGS (the two knobs: through the environment); changes
                   how a wave works and never the image.
                   `rows`: (value, scene, flags beside it) on which the variant's machine code
                   differs from the default's (tests/test_jit_variants.py proves each one);
                   `frames`: the frames the GPU file renders each row at.
  instrumentation  changes what the counters mean; the counting launches alone set it.  No row.
  library-build    read only by the library's static kernels (wo_tracers.h ...): a second build of the
                   library, out of scope.  Listed so that the completeness test knows them.

Scenes: a row of test_gen_scenes.CASES (48x36), a scene of csgrenderer_amd.scenes (64x36),
"slabs" (test_gpu_parity's axis-parallel boxes, 33x33) or "csg32_sky" (csg32 with all its geometry
behind the camera: every tile a sky tile).  Frames: "own", "61x35" and "13x7" (tiles cut in both
directions; the small tail tiles alone), "rank1of3" (61x35 as rank 1 of 3 in 4-row tiles).
"""
VARIANT, INSTRUMENTATION, LIBRARY_BUILD = "variant", "instrumentation", "library-build"
OWN = ("own",)
BLOCK_FRAMES = ("own", "61x35", "13x7", "rank1of3")


def _v(values, scenes, frames=OWN, needs="", rows=()):
    """Every value on every scene (a name, or (name, flags beside it)), and further `rows` of one
    value each.  `needs`: flags the variant only acts beside (joined to every row's own)."""
    pairs = [(s, "") if isinstance(s, str) else tuple(s) for s in scenes]
    return {"class": VARIANT, "rows": tuple((v, s, x) for v in values for s, x in pairs) + tuple(rows),
            "frames": frames, "needs": needs}


def _i(reason):
    return {"class": INSTRUMENTATION, "reason": reason}


def _l(reason="read by the library's static kernels alone"):
    return {"class": LIBRARY_BUILD, "reason": reason}


W2 = "-DWO_WINDOW=2"           # a register window of 2 events: overflow and re-collect on most rays
LDS = "-DWO_JIT_LDS_EVENTS=1"  # the event list in LDS (every scene defaults to the register window)
LDS2 = LDS + " -DWO_LDS_EVENTS=2"
NOBATCH = "-DWO_SWEEP_BATCH=0"  # the event loop where a one-word scene defaults to the batch sweep
TERM_ROWS = ("term_33", "term_64", "ties_term")
# one row per root-evaluation form (decision lists at and across the word boundary, tables beside
# lists, flat over two words, levelled tables), and flat_w2 again with overflow and re-collect
WINDOW_ROWS = ("chain_32", "chain_33", "dl_lut", "flat_w2", "hlut_regs", ("flat_w2", W2))
# the tree collect's own switches: the truth-table and levelled-table forms alone have them
RTREE_ROWS = ("dl_lut", "lut_long_term", "ties_nest", "hlut_regs", "csg32_nested", ("dl_lut", W2))
# the batch sweep: one membership word, no levelled tables (flat, lut, dl, dl + lut; ties)
BATCH_ROWS = ("flat_w1", "lut_long_term", "chain_32", "dl_lut", "ties_nest")
BLOCK_SCENES = ("csg32", "flat_w1")

TABLE = {
    # ---- term mode's literals --------------------------------------------------------------------
    "WO_TERM_F32": _v((0,), TERM_ROWS),
    "WO_LONE_SEL": _v((0,), TERM_ROWS + ("one_prim",)),
    # the event-list forms' lone spheres (term mode has no such text).  "flip": the value opposite
    # to the source's default, 0 under the union count and 1 elsewhere
    "WO_LONE_SEL_EV": _v(("flip",), ("pairs_65", "ucount_95", "flat_w1", "chain_33", "csg32_nested")),
    # ---- axis-parallel plane pairs (the generated rows rotate their operands: no pair) ---------
    "WO_AXIS_PAIR_OPAQUE": _v((0,), ("csg32", "csg32_nested", "slabs")),
    "WO_AXIS_PAIR_UNIFORM": _v((1,), ("csg32", "csg32_nested", "slabs")),
    # ---- the register window --------------------------------------------------------------------
    "WO_WINDOW": _v((2,), ("flat_w2", "dl_lut")),
    "WO_WIN_F64": _v((0,), WINDOW_ROWS),
    "WO_WIN_SELECT": _v((1,), WINDOW_ROWS, needs="-DWO_WIN_F64=1"),
    "WO_JIT_CULL_BARRIER": _v(("flip",), WINDOW_ROWS),
    "WO_WINDOW_BEYOND": _v((1,), RTREE_ROWS, needs="-DWO_JIT_LDS_EVENTS=0"),
    "WO_RECOLLECT_BEHIND": _v((0,), RTREE_ROWS),
    # ---- the sweep ------------------------------------------------------------------------------
    # (a second event per trip of the event loop: alone where the loop is the default -- two words
    # or more, levelled tables -- and beside the switches that bring the loop back elsewhere)
    "WO_SWEEP_UNROLL": _v((1,), ("chain_33", "flat_w2", "hlut_regs", ("flat_w1", NOBATCH), ("lut_long_term", NOBATCH),
                                 ("ties_nest", NOBATCH), ("flat_w1", LDS2), ("ties_nest", LDS2), ("flat_w2", W2))),
    "WO_SWEEP_BATCH": _v((0,), BATCH_ROWS),
    "WO_SWEEP_BATCH_EXIT": _v((0,), BATCH_ROWS + (("dl_lut", W2),)),
    # ---- root evaluation ------------------------------------------------------------------------
    "WO_JIT_LUT": _v((0,), ("lut_long_term", "ties_nest")),
    "WO_HBITS_LDS": _v(("flip",), ("hlut_regs", "hlut_4w")),
    # ---- the event list in LDS ------------------------------------------------------------------
    "WO_JIT_LDS_EVENTS": _v((1,), ("flat_w1", "ties_nest", "csg32_nested")),
    "WO_LDS_EVENTS": _v((2,), (("flat_w1", LDS), ("csg32_nested", LDS))),
    "WO_LDS_INSERT_UNIFORM": _v((0,), (("flat_w1", LDS), ("flat_w2", LDS), ("ties_nest", LDS), ("flat_w1", LDS2),
                                       ("flat_w2", LDS2), ("ties_nest", LDS2))),
    # (eager reads are clamped to the list: at WO_LDS_EVENTS=2 a 7 is the default's 2, only 0 differs)
    "WO_LDS_NEXT_EAGER": _v((0, 7), (("ties_nest", LDS), ("csg32_nested", LDS)), rows=((0, "flat_w1", LDS2),)),
    "WO_LDS_KEEP_SMALLEST": _v((0,), (("ties_nest", LDS2), ("csg32_nested", LDS2))),
    # ---- the block: job queue, camera iterations, row map, tail ----------------------------------
    "WO_CAM_WAVES": _v((0,), BLOCK_SCENES, BLOCK_FRAMES),  # (2 was a mode once: a static_assert refuses it)
    "WO_ROWS_LDS": _v((0,), BLOCK_SCENES + ("csg32_sky",), BLOCK_FRAMES),  # (also turns the sky loop off)
    "WO_TAIL_LDS": _v((0,), BLOCK_SCENES, BLOCK_FRAMES),
    "WO_TAIL_FRESH_LANE": _v((0,), BLOCK_SCENES, BLOCK_FRAMES),
    "WO_FRAME_SCALAR_COPIES": _v((0,), BLOCK_SCENES, BLOCK_FRAMES),
    "WO_SHADE_PRIO": _v((1,), BLOCK_SCENES, BLOCK_FRAMES),
    "WO_JIT_MIN_WAVES": _v((4,), BLOCK_SCENES, BLOCK_FRAMES),
    "WO_CAM_TILE_CULL": _v((0,), ("csg32", "term_64"), ("own", "61x35")),
    "WO_CAM_SKY_TILES": _v((0,), ("csg32", "csg32_sky"), ("own", "61x35")),
    "WO_SKY_RAYS": _v((0, 1), ("csg32",)),
    "WO_SKY_RAYS_BOUNCE_MIN": _v((1, 20), ("csg32",)),
    # ---- maths ----------------------------------------------------------------------------------
    "WO_SQRT_PT_ASM": _v((0,), ("csg32", "one_prim")),
    "WO_IEEE_SQRT": _v((1,), ("csg32", "one_prim")),
    "WO_SPHERE_SKIP": _v((0,), ("csg32", "csg32_nested")),  # (a lone sphere has no further member to skip)
    # ---- knobs that rewrite the generated source (set in the environment) ------------------------
    # the tree collect's smallest tested subtree (the table forms: default 4, levelled 2); 0: off
    "WOLOLO_JIT_RCULL": _v((0, 16), ("csg32_nested", "lut_long_term", "hlut_regs"),
                           rows=((2, "csg32_nested", ""), (2, "lut_long_term", ""), (4, "hlut_regs", ""))),
    # the spatial collect: the event-list forms without a tree collect (term mode ignores it);
    # on by default up to 64 primitives and for deep trees
    "WOLOLO_JIT_SPATIAL": _v((), (), rows=((0, "flat_w1", ""), (0, "chain_33", ""), (0, "csg256_chain", ""),
                                           (1, "pairs_65", ""))),
    # ---- instrumentation ------------------------------------------------------------------------
    "WO_COUNT_WORK": _i("the counting kernel of wo_renderer_count_work: its slots hold work counters"),
    "WO_TIME_SECTIONS": _i("cycle stamps into the counting kernel's slots"),
    "WO_SKY_RAYS_PROBE": _i("tools/sky_ray_share.py's probes: the segment counter counts something else"),
    # ---- the static kernels' own switches ---------------------------------------------------------
    **{"WO_LANES_" + n: _l() for n in (
        "TERM2", "PRIO", "PRIO_LEAF", "PRIO_TERM", "FUSED_SPHERE", "GWIN", "TRIP_NODES", "TRIP_LEAVES", "MIN_WAVES",
        "BVH_MIN_WAVES", "TERMS_MIN_WAVES", "DYN_MIN_WAVES", "DYN_TERMS_MIN_WAVES", "GENERAL_MIN_WAVES")},
}
# WO_SHADE_PRIO is also what the library's own build of the static kernels reads (wo_tracers.h
# sets its default before the shared header): that use is library-build, the row above is the
# specialised kernel's.
ALSO_LIBRARY_BUILD = ("WO_SHADE_PRIO",)
# knobs of scene_jit.c that other files test
KNOBS_TESTED_ELSEWHERE = ("WOLOLO_JIT_FLAGS", "WOLOLO_JIT_CACHE", "WOLOLO_JIT_MAX_PRIMS", "WOLOLO_JIT_GENERAL")
