"""Two-phase run-keyed merge join + aggregate (the MI355X form of a co-located bucketed
SortMergeJoin whose right key is unique: JoinIndexRule.scala:63-69).

The left key is in its run-length form (exec/encoding.RunCompact: per 64-row group a run-start
mask ``gmask`` and the first row's run ``gruns``, plus one key per run ``runkeys``).  Instead of
one kernel that stages, matches and aggregates per tile, the join is split by what each phase
streams:

1. ``hs_jit_run_tags`` - per merge-join tile, the tile's right key span is staged in LDS with
   the right side's predicates evaluated once per right row; each thread matches a contiguous
   chunk of the tile's runs (one LDS binary search, then a walk) and writes a W-bit **tag** per
   run into a bitmap: 0 = no (passing) right row, else 1 (ungrouped / left-grouped) or the
   right-side group code + 1.  Tags are assembled in LDS and leave as whole 32-bit words (only
   a tile's two edge words use an atomic OR).  It reads the run keys, the right keys and the
   right predicate columns once: 10 B per run (4 + 4 + 2), 1.5 GB over the 150 M runs of TPC-H
   SF100 Q3, in ~0.30 ms beside the Q6 scan - 5.0 TB/s one run per lane, 5.2 TB/s four
   (``profiles/tags2_wide.txt``; a FETCH_SIZE counter pass reads about half of these computed
   bytes for all three query kernels, ``profiles/pmc_query_kernels_sf100_r6.txt``).
2. ``hs_jit_run_scan`` - a streaming scan of the left rows (vector loads, no LDS staging, no
   barriers): row -> run index from the group mask by one popcount, tag from the bitmap (the
   NI rows of a thread touch one or a few adjacent words), left predicates, and the compacted
   aggregate tail over the passing rows only.

Both phases are plain streams (phase 2 at ~5.8 TB/s of its computed bytes; the three kernels
of a headline step together move ~4.0 GB in 0.70 ms, 5.7 TB/s); the single-kernel form
(jit.gen_merge_join_agg) keeps a long chain of dependent round trips per tile.

The pruned pair (``prune_plan``, RS_PRUNE; the headline Q3's form) reads fewer bytes: phase 1
also loads one per-run bound of the left predicate column (2 B per run: 12 B per run, 1.8 GB)
and clears the tags of runs no row of which can pass, and phase 2 (``hs_jit_run_bits_cand``)
drops its row stream - the 0.9 GB 12-bit ``l_shipdate`` copy - and gathers the tail words of the
tagged runs' rows only (1.35 instead of 1.27 128-byte lines per 100 left rows): ~1.0 GB
instead of ~1.9.  The step moves ~3.45 GB in 0.68 ms (5.1 TB/s): phase 1 369 us (4.9 TB/s),
phase 2 256 us - a gather, not a stream, so below the streaming rate
(``profiles/run_prune.txt``).

With 16-bit key offsets (RT2_K16, ``tags2_k16``; the default) the four-run phase 1 reads both
key columns as uint16 offsets from the bases of 32-element groups (``encoding.group16_32``,
built natively by ``hs_group16_32``; exact: code = base + offset): 8.25 instead of 12 B per run,
1.24 GB, and the step moves ~2.9 GB in 0.585 ms (5.0 TB/s; phase 1 377 -> 264 us at 4.7 TB/s,
``profiles/tags2_keys16.txt``).  The 32-bit arrays stay resident for the gallop and for stages
that meet a wide group.

Phase 1 streams the same 1.24 GB for every query of a shape - only the literal compares at its
end differ - so that form can tag two queries in one pass (RT2_PAIR, ``tags2_pair``;
``TwoPhaseLauncher.launch_pair``): a second set of literal slots, a second bitmap (19 MB), and
everything literal-independent done once per run.  ``exec/pairing.py`` pairs a query submitted
asynchronously while its predecessor still runs with the next one of the lowering; each keeps
its own phase 2, final reduction and result copy, so its result is bit for bit the unpaired
one.  Phase-1 dispatches per headline step 1.0 -> 0.55, step 0.592-0.595 -> 0.480-0.503 ms
(medians 0.594 -> 0.486; ``profiles/tags2_pair.txt``).

The candidate phase 2 gathers nearly the same tail-word lines for both queries of a pair (their
candidate bands overlap by 121 of 128 days or more), so it has a pair form too (RS_PAIR,
``cand_pair``; kernel ``hs_jit_run_bits_cand2``): per tile both row masks, one gather over the
union of the two candidate sets, each query's own predicate test, list, walk, accumulators and
block partials - bit for bit the single launches' (``gen_run_sparse_scan``).  A pair is then
pair phase 1, pair phase 2, and per query the final reduction and result copy
(``profiles/bits_cand_pair.txt``).

Both candidate forms keep a passing row's tail word where the filter pass has it (RS_KEEP): it
goes into a per-wavefront LDS ring of 63 + 64 RS_WALK entries instead of its row offset into a
list, and the sums are taken from the ring in whole groups of 64 entries after every pass, the
rest where the listing form walked.  The walk then loads nothing: one memory round trip per
tile and query less, 12.7 / 22.8 KB of LDS per workgroup (single / pair), and the single form
drops from 70 to 62 VGPRs (eight waves per SIMD).  Pair dispatch 450 -> 406 us, single
217 -> 200 us, step 0.460 -> 0.438 ms: a tenth of the kernels' time, not the quarter one trip
less was expected to give - the reload was an L2 hit (``profiles/bits_cand_keep.txt``).  The
two-phase
form applies when no aggregate input comes from the right side, every right predicate reads
only right columns, and a right-side group key (if any) has at most 255 groups."""
from __future__ import annotations

import collections
import re
from typing import List, Optional

from ..ops import _lib as NL
from . import jit as J
from . import jit_hash as JH

SPLIT = 8
# tunables: fields of exec.kernel_config.KernelConfig (bound by kernel_config.bind)
from . import kernel_config as _KC  # noqa: E402
_CFG = _KC.active()
MJ_2P, RS_ITEMS = _CFG.mj_2p, _CFG.rs_items
RT2_UNROLL, RT2_GRID, RT2_I32 = _CFG.rt2_unroll, _CFG.rt2_grid, _CFG.rt2_i32
RT2_MATCH, RT2_COPY, RT2_LO16 = _CFG.rt2_match, _CFG.rt2_copy, _CFG.rt2_lo16
RT2_WIDE, RT2_WIDE_GRID, RT2_K16 = _CFG.rt2_wide, _CFG.rt2_wide_grid, _CFG.rt2_k16
RT2_PAIR = _CFG.rt2_pair
RS_BITS, RS_BITS_GRID, RS_PACK = _CFG.rs_bits, _CFG.rs_bits_grid, _CFG.rs_pack
RS_PIPE, RS_WALK, RS_LDS, RS_LUT = _CFG.rs_pipe, _CFG.rs_walk, _CFG.rs_lds, _CFG.rs_lut
RS_PK16, RS_WAVES, RS_PACK12 = _CFG.rs_pk16, _CFG.rs_waves, _CFG.rs_pack12
RS_PRUNE, RS_PAIR, RS_KEEP = _CFG.rs_prune, _CFG.rs_pair, _CFG.rs_keep


def tag_width(p: NL.JoinParams) -> int:
    """Bits per run tag, or 0 when the two-phase form does not apply to ``p``."""
    if p.group_col >= SPLIT:
        if p.num_groups > 255:
            return 0
        for w in (1, 2, 4, 8):
            if p.num_groups + 1 <= (1 << w):
                return w
    return 1


def applies(p: NL.JoinParams) -> bool:
    if not MJ_2P or J.has_guards(p):
        # (the two phases carry one pass bit per row: a guarded aggregate takes the generic
        # merge join, whose aggregate phase sees the guard's columns)
        return False
    for i in range(p.naggs):
        a = p.aggs[i]
        if any(a.col[t] >= SPLIT for t in range(a.nterms)) and a.kind != NL.AK_COUNT_STAR:
            return False
    if not J._right_only(p, SPLIT):
        return False
    if p.group_col >= SPLIT and p.cols[p.group_col].valid:
        return False
    return tag_width(p) > 0


def _rpreds(p):
    return [(k, p.preds[k]) for k in range(p.nlp, p.npreds)]


def _lpreds(p):
    return [(k, p.preds[k]) for k in range(p.nlp)]


# phase 1: 64-run groups per unrolled iteration of a wavefront (gen_run_tags2)


def tags2_wide(p: NL.JoinParams, compacts, ix32: bool, mode: str = "") -> int:
    """Runs per lane of phase 1 for this join (the lowering's choice): RT2_WIDE's 4-run form
    only for the verifying kernel (modes "" and "rec") with 32-bit indices, and only when the
    right key and every staged right column are stored plainly or as a one-array compact code
    without a validity mask - the grouped 16-bit key encoding and nullable columns keep the
    one-run form, which reads them element by element."""
    if RT2_WIDE != 4 or not ix32 or mode not in ("", "rec"):
        return 1
    cols = J._col_specs(p, compacts)
    for sl in dict.fromkeys([p.rkey] + _stage_slots(p)):
        enc = cols[sl][2]
        if cols[sl][1] or (enc and len(enc) > 2 and enc[2] == 64):
            return 1
    return 4


# the share of a key column's 32-element groups that may be wide before its 16-bit form is
# refused (``key_forms16``): a stage that meets a wide group falls back to the 64-run code
K16_MAX_WIDE = 0.03


def tags2_k16(p: NL.JoinParams, compacts, ix32: bool, mode: str = "") -> bool:
    """Whether phase 1 of this join may read its two key columns as 16-bit offsets from
    32-element group bases (RT2_K16): the four-run form in mode "" whose right key is a plain
    32-bit compact code (not nullable, not already stored grouped: ``tags2_wide`` refuses
    those) and whose left key has the run form.  The lowering still needs both derived forms
    (``key_forms16``) before it picks the variant."""
    if not RT2_K16 or RT2_LO16 or mode != "" or tags2_wide(p, compacts, ix32, mode) != 4:
        return False
    lc, rc = (compacts or {}).get(p.lkey), (compacts or {}).get(p.rkey)
    return lc is not None and lc.signature() == (4, False, "runs") and \
        rc is not None and rc.signature() == (4, False)


# the right key's 16-bit form: id of its codes -> (weak reference to the codes, (offsets, bases)
# or None).  Derived once per resident table, like the per-run bounds below, and dropped with the
# codes (an evicted table's are not kept alive here); the left key's is kept on its RunCompact
# (``keys16``).
_KEYS16: dict = {}


def key_forms16(runs, rc) -> Optional[tuple]:
    """((left offsets, left bases), (right offsets, right bases)) of the run keys of ``runs``
    and the right key compact ``rc`` over 32-element groups (``encoding.group16_32``), or None
    when either side has more than K16_MAX_WIDE wide groups."""
    from . import encoding as E
    from .device_cache import track_derived
    lf = runs.keys16(K16_MAX_WIDE, E.GROUP32)
    if lf is None:
        return None
    import weakref
    key = id(rc.codes)
    hit = _KEYS16.get(key)
    if hit is None or hit[0]() is not rc.codes:
        rf = E.group16_32(rc.codes, K16_MAX_WIDE)
        if rf is not None and rc.codes.is_cuda:
            for t in rf:
                track_derived(t)
        hit = _KEYS16[key] = (weakref.ref(rc.codes), rf)
        weakref.finalize(rc.codes, _drop_keys16, key, hit)
    return None if hit[1] is None else (lf, hit[1])


def _drop_keys16(key: int, entry: tuple) -> None:
    if _KEYS16.get(key) is entry:       # (the id may have been reused by a live tensor)
        del _KEYS16[key]


def tags2_pair(p: NL.JoinParams, compacts, W: int, ix32: bool, mode: str = "",
               k16: bool = False) -> bool:
    """Whether phase 1 of this join has the pair form (RT2_PAIR): one pass over the keys, the
    right predicate columns and the run bounds tags two queries of the shape, each with its own
    literal slots and bitmap.  Only the headline's form: the verifying four-run kernel over
    16-bit key offsets (``tags2_k16``: mode ""), 1-bit tags, with or without ``prune_plan``
    bounds."""
    return bool(RT2_PAIR and W == 1 and mode == "" and k16 and
                tags2_k16(p, compacts, ix32, mode))


# the second literal set of the pair form: slot name + this suffix
PAIR_SFX = "_b"


def tags2_shape(p: NL.JoinParams, compacts, W: int, ix32: bool = False, mode: str = "",
                prune: tuple = (), k16: bool = False, pair: bool = False) -> tuple:
    cols = tuple(sorted((s, c) for s, c in J._col_specs(p, compacts).items()
                        if s >= SPLIT or s == p.lkey))
    preds = J._preds_shape(p, p.nlp, p.npreds)
    return ("run_tags2", cols, preds, p.nlp, p.lkey, p.rkey, _tags_grouped(p) and p.group_col,
            W, RT2_UNROLL, J.BLOCK, ix32, mode, tuple(prune),
            bool(k16) and tags2_k16(p, compacts, ix32, mode),
            bool(pair) and tags2_pair(p, compacts, W, ix32, mode, k16),
            tags2_wide(p, compacts, ix32, mode))


def prune_plan(p: NL.JoinParams, compacts, W: int, hk=None, record: bool = False) -> tuple:
    """The left conjuncts phase 1 pre-filters by per-run bounds (RS_PRUNE), as ((predicate
    index, column slot, uses the run's maximum), ...) - or () when the pruned pair of kernels
    does not apply and the join keeps the streaming phase 2.

    It applies to the plain-aggregate, 1-bit-tag, verifying form (``hk`` None, no recorded
    match, no left group key) when every left predicate is a conjunct of its own comparing a
    non-nullable 16-bit compact column with a literal by <, <=, > or >= in code space (the
    CL<k> / CH<k> bounds of ``fill_preds_aggs``; an IS NOT NULL conjunct on a non-nullable
    column holds for every row and is passed over), and those columns' codes fit the row-packed
    tail word beside the aggregate inputs (``pack_layout`` with ``extra``).  A run can hold a
    passing row only if its largest code reaches CL (>, >=) or its smallest stays within CH
    (<, <=): conservative for any literal, and phase 2 still tests every candidate row exactly."""
    if not (RS_PRUNE and RS_BITS) or W != 1 or hk is not None or record or _scan_grouped(p):
        return ()
    out, groups = [], set()
    for k, pr in _lpreds(p):
        if pr.kind == NL.PK_TRUE:
            continue
        if pr.group in groups or p.cols[pr.col].valid:
            return ()
        groups.add(pr.group)
        if pr.kind == NL.PK_NOT_NULL:       # holds for every row of a non-nullable column
            continue
        c = (compacts or {}).get(pr.col)
        if c is None or \
                type(c).__name__ != "Compact" or c.width != 2 or getattr(c, "runs", None):
            return ()
        if pr.op not in (NL.OP_LT, NL.OP_LE, NL.OP_GT, NL.OP_GE):
            return ()
        if not ((pr.kind == NL.PK_INT_LIT and c.scale is None) or
                (pr.kind == NL.PK_FLT_LIT and c.scale is not None)):
            return ()
        out.append((k, pr.col, pr.op in (NL.OP_GT, NL.OP_GE)))
    if not out or pack_layout(p, compacts, tuple(dict.fromkeys(sl for _, sl, _ in out))) is None:
        return ()
    return tuple(out)


# a literal slot of ``fill_preds_aggs`` in generated source (predicate k's value / bounds / set)
_LIT_SLOT = re.compile(r"\ba\.((?:CL|CH|L|F|T|U|S|N)\d+)\b")
# ... and of phase 2: also the aggregate coefficients A<i>_<t> / B<i>_<t>; its partial pointers
# and accumulator registers (the pair form's second query gets twins of all three)
_LIT_SLOT2 = re.compile(r"\ba\.((?:CL|CH|L|F|T|U|S|N)\d+|[AB]\d+_\d+)\b")
_PART_SLOT = re.compile(r"\ba\.(psum|pcnt|pmin|pmax)\b")
_ACC_REG = re.compile(r"\b(acc|cnt)(\d+)\b")


def _stage_slots(p: NL.JoinParams) -> list:
    """Right columns phase 1 reads at a matched row: predicate columns and the group key."""
    return list(dict.fromkeys(J._pred_slots(_rpreds(p)) +
                              ([p.group_col] if _tags_grouped(p) else [])))


def _tags_grouped(p: NL.JoinParams) -> bool:
    """Whether the tags carry a right-side group code: a right group key with more than one
    group (a single group's domain [group_base, group_base + 1) holds every value of the column,
    which is non-null here: ``applies``)."""
    return p.group_col >= SPLIT and p.num_groups > 1


# Which phase-1 kernel is generated, resolved once (``_tags_form``): its name; the run /
# right-row index type IX; tag bits W with MASK and L, the lanes whose 4 tags share one 32-bit word
# in the four-run form; runs per lane ``wide`` (``tags2_wide``); U, the 64-run groups per iteration
# or 256-run blocks per pipeline stage; whether it records the match (``rec``), reads a recorded
# match (``match``) or per-run column copies (``copy``), compares 16-bit key halves (``lo16``) or
# prepares them (``prep``); ``k16`` / ``pair``; whether the tags carry a right-side group code
# (``rgroup``) and the right key is stored grouped (``rkg``); the right columns read at a matched
# row; and per pre-filter conjunct (bound array slot, literal slot, comparison).
_TagsForm = collections.namedtuple(
    "_TagsForm", "name IX W MASK L wide U rec match copy lo16 prep k16 pair rgroup rkg "
                 "stage_slots bounds")


def _tags_form(p: NL.JoinParams, compacts, W: int, ix32: bool, mode: str, prune: tuple,
               k16: bool, pair: bool) -> _TagsForm:
    """The form of ``gen_run_tags2``'s arguments under the bound tunables, and every check that
    the combination exists.  The only place that looks at ``mode``.

    ``ix32``: run and right-row indices fit int32 (the lowering checks the table sizes), so the
    index arithmetic, range clamps and gallop run in 32-bit registers and the column loads
    address through a scalar base plus a 32-bit lane offset - the 64-bit index math was most of
    the kernel's VALU instructions (``profiles/pmc_query_kernels_sf100_r6.txt``)."""
    assert not prune or mode == ""
    assert not k16 or tags2_k16(p, compacts, ix32, mode)
    assert not pair or tags2_pair(p, compacts, W, ix32, mode, k16)
    recorded, lo16 = mode in ("match", "copy"), mode in ("lo16", "lo16prep")
    assert ix32 or recorded or not (mode == "rec" or lo16)
    wide = tags2_wide(p, compacts, ix32, mode)
    # four-run form: 256-run blocks per pipeline stage (RT2_UNROLL counts blocks there), at most
    # two - 84 VGPRs at W = 1, six waves per SIMD; a third block's register sets would spill
    U = max(1, min(2, RT2_UNROLL) if wide == 4 else RT2_UNROLL)  # noqa: N806
    stage_slots = _stage_slots(p)
    enc = J._col_specs(p, compacts)[p.rkey][2]
    rkg = not recorded and bool(enc and len(enc) > 2 and enc[2] == 64)
    assert not rkg or p.rkey not in stage_slots
    bounds = tuple((f"RMX{sl}" if mx else f"RMN{sl}", f"CL{k}" if mx else f"CH{k}",
                    ">=" if mx else "<=") for k, sl, mx in prune)
    return _TagsForm("hs_jit_key_lo16" if mode == "lo16prep" else "hs_jit_run_tags2",
                     "int" if ix32 else "i64", W, (1 << W) - 1, 8 // W, wide, U, mode == "rec",
                     mode == "match", mode == "copy", lo16, mode == "lo16prep", bool(k16),
                     bool(pair), _tags_grouped(p), rkg, stage_slots, bounds)


class _Tags2:
    """The builder behind ``gen_run_tags2``: one method per stage of the kernel, each returning
    its source lines, over the form ``f``, the argument struct and the column descriptions.

    The verifying kernel has no tiles and no LDS.  Each wavefront owns a contiguous chunk of
    64-run groups of the left run list (so it owns whole 2W-word stretches of the tag bitmap and
    stores them without atomics).  Ranges (``RNG``, NRG x 4 int64, sorted by first run):
    [first run, end run) of each left row range and the right bucket's rows [s0, s1).  (16-bit
    grouped run keys measured 0.59 vs 0.29 ms - more dependent loads per run - and a per-tile
    LDS form 0.79 ms: both removed.)

    Stages add slots to ``args`` as they emit, and the slot order is the ``Args`` struct layout -
    part of the source text - so the order of the driver's calls is fixed: ``header`` (every
    slot that does not depend on a column's encoding), ``images`` (the right key's validity
    pointer, group_base / num_groups, the key's pointers and base, ``NRIGHT``), then the loop
    top to bottom - ``group`` / ``load`` / ``recorded_loads`` add the staged columns' pointers and
    bases (the copy form its ``S<slot>`` / ``SV<slot>``) at their first load, ``tag_expr`` the
    right predicates' literal slots, and ``lit_b`` a ``PAIR_SFX`` twin of every literal slot
    where the second set first names it, so straight after the first tag expression's own."""

    def __init__(self, p: NL.JoinParams, compacts, W: int, ix32: bool, mode: str, prune: tuple,
                 k16: bool, pair: bool):
        self.f = _tags_form(p, compacts, W, ix32, mode, prune, k16, pair)
        self.p, self.lk, self.rk = p, p.lkey, p.rkey
        self.args = J.Args()
        self.cols = J._col_specs(p, compacts)
        self.rpreds = _rpreds(p)
        self.WV = J.BLOCK // 64

    def gen(self, row: str) -> J._Gen:
        return J._Gen(self.args, self.cols, SPLIT, (row, row), frozenset(), True)

    def header(self) -> None:
        """The argument slots that precede the columns'."""
        f, add = self.f, self.args.add
        if f.match or f.copy:
            add("p", *(("HIT", "const u64*") if f.copy else ("MATCH", "const int*")))
            add("p", "tags", "unsigned*")
            add("q", "NRUNS", "long long")
            self.group_args()
            return
        add("p", f"RK{self.lk}", "const int*")
        add("p", "RNG", "const long long*")
        add("p", "tags", "unsigned*")
        if f.pair:
            add("p", "tags" + PAIR_SFX, "unsigned*")
        for n in ("NRG", "NRUNS", "KLO", "KSP", "KOF"):
            add("q", n, "long long")
        if f.rec:
            add("p", "MOUT", "int*")
        for arr, lit, _ in f.bounds:
            add("p", arr, "const unsigned short*")
            add("q", lit, "long long")
        if f.k16:
            for n in ("LO16", "RO16"):
                add("p", n, "const unsigned short*")
            for n in ("LG16", "RG16"):
                add("p", n, "const int*")
        if f.lo16:
            cst = "" if f.prep else "const "
            add("p", "LL", f"{cst}unsigned short*")
            add("p", "RL", f"{cst}unsigned short*")

    def group_args(self) -> None:
        if self.f.rgroup:
            self.args.add("q", "group_base", "long long")
            self.args.add("q", "num_groups", "long long")

    def images(self) -> List[str]:
        """The lambdas from a right row to its 32-bit key image (the left images are run key +
        KOF): ``IMG``, exact; ``IMGF``, the guess's, and ``IMGV`` (four-run form), from a loaded
        element.  Adds the right key's slots and, between its validity pointer and the rest,
        group_base / num_groups."""
        f, args, rk = self.f, self.args, self.rk
        g = self.gen("row_")
        rv = J._valid_expr(g, rk, "row_")
        self.group_args()
        if f.rkg:
            # grouped 16-bit right key: code = gbase[row >> 6] + offset, or the 32-bit code of a
            # wide group (both loads unconditional: the wide one hits row 0 otherwise)
            base = args.add("q", f"B{rk}", "long long")
            gp = args.add("p", f"G{rk}", "const int*")
            wp = args.add("p", f"W{rk}", "const int*")
            cp = g.ptr(rk)
            rval = (f"({{ const int gb_ = {gp}[row_ >> 6]; const bool wd_ = gb_ == (int)0x80000000; "
                    f"const int w_ = {wp}[wd_ ? row_ : 0]; const unsigned short o_ = {cp}[row_]; "
                    f"{base} + (wd_ ? (i64)w_ : (i64)gb_ + (i64)o_); }})")
            # the guess's image without the dependent wide-group load: 0 (below every left image,
            # so never a false match) for a wide group; a miss re-reads the exact image
            fval = (f"({{ const int gb_ = {gp}[row_ >> 6]; const unsigned short o_ = {cp}[row_]; "
                    f"gb_ == (int)0x80000000 ? (i64)-1 : {base} + (i64)gb_ + (i64)o_; }})")
        else:
            rval = fval = g.value(rk, "row_")

        def image(val: str, wide0: bool) -> str:
            guard = "(__v_ == (i64)-1) || " if wide0 else ""
            return (f"({rv} ? 0u : ({{ const i64 __v_ = (i64)({val}); const i64 d_ = __v_ - a.KLO; "
                    f"({guard}d_ < 0) ? 0u : (d_ > a.KSP ? 0xFFFFFFFFu : (unsigned)(d_ + 1)); }}))")
        b = [f"  auto IMG = [&]({f.IX} row_) -> unsigned {{ return {image(rval, False)}; }};"]
        if f.prep:
            args.add("q", "NRIGHT", "long long")
            return b
        b.append(f"  auto IMGF = [&]({f.IX} row_) -> unsigned "
                 f"{{ return {image(fval, fval is not rval)}; }};")
        if f.wide == 4:
            b.append(f"  auto IMGV = [&]({g.raw_type(rk)} w_) -> unsigned "
                     f"{{ return {image(g.decode(rk, 'w_'), False)}; }};")
        return b

    def prep_body(self) -> List[str]:
        """The low 16 bits of every left run key image and right key image (``lo16_keys``)."""
        return [f"  const i64 t_ = (i64)blockIdx.x * {J.BLOCK} + threadIdx.x, "
                f"n_ = (i64)gridDim.x * {J.BLOCK};",
                f"  for (i64 i = t_; i < a.NRUNS; i += n_) "
                f"a.LL[i] = (unsigned short)((unsigned)a.RK{self.lk}[i] + (unsigned)a.KOF);",
                "  for (i64 i = t_; i < a.NRIGHT; i += n_) a.RL[i] = (unsigned short)IMG((int)i);"]

    def prologue(self) -> List[str]:
        """A wavefront's chunk [gbeg, gend) of 64-run groups - in the four-run form [bbeg, bend)
        of 256-run blocks, in int, whole stages per wavefront so only a chunk's last stage can
        be cut by its end - all wavefront-uniform (scalar registers, scalar loads of the range
        table)."""
        f = self.f
        blocks = f.wide == 4
        T, N, x = ("int", "NB", "b") if blocks else ("i64", "G", "g")  # noqa: N806
        cast = "" if blocks else "(i64)"
        per = f"(({N} + nwv - 1) / nwv + {f.U - 1}) / {f.U} * {f.U}" if blocks else \
            f"({N} + nwv - 1) / nwv"
        return ["  const int lane = (int)(threadIdx.x & 63);",
                "  const i64 G = (a.NRUNS + 63) >> 6;"] + \
            (["  const int NR = (int)a.NRUNS, NB = (int)((a.NRUNS + 255) >> 8);"]
             if blocks else []) + [
                f"  const {T} nwv = ({T})gridDim.x * {self.WV};",
                f"  const {T} wv = ({T})blockIdx.x * {self.WV} + "
                f"{cast}__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));",
                f"  const {T} per = {per};",
                f"  const {T} {x}beg = wv * per;",
                f"  const {T} {x}end = {N} < {x}beg + per ? {N} : {x}beg + per;"] + \
            ([] if f.match or f.copy else [f"  if ({x}beg >= {x}end || a.NRG <= 0) return;"]) + \
            (["  const i64 gend = G < ((i64)bend << 2) ? G : ((i64)bend << 2);"] if blocks else [])

    def seek(self) -> List[str]:
        """The range of the chunk's first run (a binary search of the range table) and the guess
        base."""
        IX, blocks = self.f.IX, self.f.wide == 4  # noqa: N806
        return ["  const i64* RG = a.RNG;",
                "  int rg = 0;",
                "  { int lo = 0, hi = (int)a.NRG; const i64 r0 = " +
                ("(i64)bbeg << 8" if blocks else "gbeg << 6") + ";",
                "    while (hi - lo > 1) { const int m = (lo + hi) >> 1; "
                "if (RG[4 * m] <= r0) lo = m; else hi = m; }",
                "    rg = lo; }",
                f"  {IX} lr0 = ({IX})RG[4 * rg], lr1 = ({IX})RG[4 * rg + 1], "
                f"s0 = ({IX})RG[4 * rg + 2], s1 = ({IX})RG[4 * rg + 3];",
                "  i64 nxt0 = rg + 1 < a.NRG ? RG[4 * (rg + 1)] : 0x7fffffffffffffffll;",
                f"  {IX} gbase = -1;   // right row of the next {'stage' if blocks else 'group'}'s "
                f"first run (-1: range-relative)"]

    def advance(self, at: str, ind: str, inline: bool = False) -> List[str]:
        """Step to the range that holds run ``at``."""
        IX = self.f.IX  # noqa: N806
        b = [f"{ind}while (nxt0 <= {at}) {{",
             f"{ind}  ++rg; lr0 = ({IX})RG[4 * rg]; lr1 = ({IX})RG[4 * rg + 1]; "
             f"s0 = ({IX})RG[4 * rg + 2];",
             f"{ind}  s1 = ({IX})RG[4 * rg + 3]; gbase = -1;",
             f"{ind}  nxt0 = rg + 1 < a.NRG ? RG[4 * (rg + 1)] : 0x7fffffffffffffffll;"]
        if inline:
            b[-1] += " }"
            return b
        return b + [f"{ind}}}"]

    def group(self, u: int, fast: bool, ind: str) -> List[str]:
        """Loads and guess of 64-run group ``gi + u``.  Lane l guesses the right row of its run:
        the previous group's last match + 1 + l (or, at a range start, the range-relative
        position) - exact for a foreign key whose every right key has left rows, the common
        case.  The right predicate and group columns are loaded at the guess together with the
        key, so a verified guess costs one round trip.  ``fast`` (every run of the iteration
        lies in range rg): unconditional (clamped) loads, so all U groups' loads are in flight
        together (a load under a per-lane condition makes the compiler wait for it before the
        branches merge).  ``prune_plan``'s bound of the run - ``RMX<slot>`` or ``RMN<slot>``,
        one uint16 per run (code + 32768, ``run_bounds``) - is loaded with the run key."""
        f, lk, IX = self.f, self.lk, self.f.IX  # noqa: N806
        b = [f"{ind}const {IX} r{u} = ({IX})(((gi + {u}) << 6) + lane);",
             f"{ind}const bool in{u} = gi + {u} < gend;"]
        if fast:
            b.append(f"{ind}const {IX} l0_{u} = lr0, l1_{u} = lr1, a0_{u} = s0, a1_{u} = s1; "
                     f"const bool own{u} = true;")
        else:
            b.extend([f"{ind}{IX} l0_{u} = lr0, l1_{u} = lr1, a0_{u} = s0, a1_{u} = s1; "
                      f"bool own{u} = true;",
                      f"{ind}if (r{u} >= nxt0) {{ own{u} = false; int q_ = rg;",
                      f"{ind}  while (q_ + 1 < (int)a.NRG && RG[4 * (q_ + 1)] <= r{u}) ++q_;",
                      f"{ind}  l0_{u} = ({IX})RG[4 * q_]; l1_{u} = ({IX})RG[4 * q_ + 1]; "
                      f"a0_{u} = ({IX})RG[4 * q_ + 2]; a1_{u} = ({IX})RG[4 * q_ + 3]; }}"])
        b.extend([f"{ind}const bool act{u} = in{u} && r{u} < a.NRUNS && r{u} >= l0_{u} && "
                  f"r{u} < l1_{u} && a1_{u} > a0_{u};",
                  f"{ind}{IX} j{u} = (own{u} && gbase >= 0) ? gbase + {u * 64} + lane : "
                  f"a0_{u} + (r{u} - l0_{u});",
                  f"{ind}j{u} = act{u} ? (j{u} < a0_{u} ? a0_{u} : (j{u} >= a1_{u} ? a1_{u} - 1 : j{u}))"
                  f" : 0;"])
        if f.lo16 and fast:
            # 16-bit key halves per lane; the full images of the group's two end pairs (lanes
            # 0 / 1 load them for lane 0 / lane 63) decide in ``resolve`` whether halves suffice
            b.extend([f"{ind}const unsigned key{u} = (unsigned)a.LL[act{u} ? r{u} : 0];",
                      f"{ind}const unsigned k{u} = (unsigned)a.RL[j{u}];",
                      f"{ind}const int j0_{u} = __builtin_amdgcn_readlane((int)j{u}, 0), "
                      f"j63_{u} = __builtin_amdgcn_readlane((int)j{u}, 63);",
                      f"{ind}const int re_{u} = (int)((gi + {u}) << 6) + ((lane & 1) ? 63 : 0);",
                      f"{ind}const unsigned fk{u} = (unsigned)a.RK{lk}[re_{u} < a.NRUNS ? re_{u} : 0]"
                      f" + (unsigned)a.KOF;",
                      f"{ind}const unsigned fi{u} = IMGF((lane & 1) ? j63_{u} : j0_{u});"])
        else:
            b.extend([f"{ind}const unsigned key{u} = (unsigned)a.RK{lk}[act{u} ? r{u} : 0] + "
                      f"(unsigned)a.KOF;",
                      f"{ind}const unsigned k{u} = IMGF(j{u});"])
        for i, (arr, _, _) in enumerate(f.bounds):
            b.append(f"{ind}const int bm{i}_{u} = (int)a.{arr}[act{u} ? r{u} : 0];")
        gu = self.gen(f"j{u}")
        for sl in f.stage_slots:
            J._uload(gu, sl, f"g{u}", b, ind)
        return b

    def lit_b(self, expr: str) -> str:
        """``expr`` over the pair's second literal set: every literal slot it names gets a twin
        (same kind and type) with ``PAIR_SFX``, added where first met."""
        def twin(m):
            kind, name, ct = self.args.slots[self.args._index[m.group(1)]]
            return self.args.add(kind, name + PAIR_SFX, ct)
        return _LIT_SLOT.sub(twin, expr)

    def tag_expr(self, gen: J._Gen, it: str, x) -> str:
        """The tag of run ``x`` from ``hit<x>`` and the right columns loaded as item ``it``: 0 =
        no (passing) right row, else 1 or the right-side group code + 1.  Adds the right
        predicates' literal slots.  (The forms over a record spell the same test with other
        parentheses.)"""
        f = self.f
        cond = J._rename(gen.cnf(self.rpreds), f.stage_slots, it)
        recorded = f.match or f.copy
        ok = f"hit{x}" if recorded else f"(hit{x})"
        if not f.rgroup:
            return f"({ok} && {cond}) ? 1u : 0u" if recorded else f"({ok} && {cond} ? 1u : 0u)"
        gx = J._rename(f"x{self.p.group_col}", f.stage_slots, it)
        return (f"({{ const i64 gl_ = (i64){gx} - a.group_base; ({ok} && {cond} && gl_ >= 0 && "
                f"gl_ < a.num_groups) ? (unsigned)(gl_ + 1) : 0u; }})")

    def resolve(self, x, ind: str, lo: bool = False) -> List[str]:
        """Verifies the guess of run ``x`` with one compare of the 32-bit key images and leaves
        ``hit<x>``, the matched row ``m<x>`` and the tag ``tg<x>`` (pair: ``tgb<x>`` for the
        second literal set - loads, guess, compare and gallop run once per run, the right
        predicates and bound tests once per set); a mismatch gallops from the guess to the lower
        bound (exact for any sorted unique right keys) and reloads the staged columns there.
        The tag is cleared when a loaded bound fails its conjunct's code range [CL<k>, CH<k>]
        (hs_c20 keeps the sum in int32).  ``lo``: the group's keys are 16-bit halves."""
        f, lk, IX = self.f, self.lk, self.f.IX  # noqa: N806
        u, b = x, []
        gu = self.gen(f"j{u}")
        # (a checked group's keys are low halves: a miss gallops with the full left key)
        kfull = f"(unsigned)a.RK{lk}[r{u}] + (unsigned)a.KOF" if lo else f"key{u}"
        if lo:
            # halves decide when every lane is active, the guesses are consecutive and both end
            # pairs match in full with a key span below 2^16: any lane's two keys then differ by
            # less than 2^16.  Otherwise every lane takes the full-key path below.
            b.extend([f"{ind}const unsigned fk0_{u} = (unsigned)__builtin_amdgcn_readlane((int)fk{u}, 0), "
                      f"fk1_{u} = (unsigned)__builtin_amdgcn_readlane((int)fk{u}, 1);",
                      f"{ind}const bool cl{u} = __ballot(act{u}) == ~0ull && j63_{u} - j0_{u} == 63 && "
                      f"fk0_{u} == (unsigned)__builtin_amdgcn_readlane((int)fi{u}, 0) && "
                      f"fk1_{u} == (unsigned)__builtin_amdgcn_readlane((int)fi{u}, 1) && "
                      f"fk1_{u} - fk0_{u} < 65536u;",
                      f"{ind}bool hit{u} = act{u} && cl{u} && k{u} == key{u};"])
        else:
            b.append(f"{ind}bool hit{u} = act{u} && k{u} == key{u};")
        b.extend([f"{ind}{IX} m{u} = j{u};",
                  f"{ind}unsigned tg{u} = {self.tag_expr(gu, f'g{u}', u)};"])
        if f.pair:
            b.append(f"{ind}unsigned tgb{u} = {self.lit_b(self.tag_expr(gu, f'g{u}', u))};")
        b.extend([f"{ind}if (act{u} && !hit{u}) {{",
                  # gallop from the guess to the lower bound of key in [a0, a1)
                  f"{ind}  const unsigned key_ = {kfull}; {IX} lo_, hi_;",
                  f"{ind}  const unsigned kj_ = IMG(j{u});",
                  f"{ind}  if (kj_ == key_) {{ lo_ = j{u}; hi_ = j{u}; }}",
                  f"{ind}  else if (kj_ > key_) {{",
                  f"{ind}    hi_ = j{u}; {IX} st_ = 1; lo_ = j{u} - 1;",
                  f"{ind}    while (lo_ > a0_{u} && IMG(lo_) >= key_) {{ hi_ = lo_; st_ <<= 1; "
                  f"lo_ = hi_ - st_; }}",
                  f"{ind}    if (lo_ < a0_{u}) lo_ = a0_{u};",
                  f"{ind}  }} else {{",
                  f"{ind}    lo_ = j{u} + 1; {IX} st_ = 1; hi_ = j{u} + 1;",
                  f"{ind}    while (hi_ < a1_{u} && IMG(hi_) < key_) {{ lo_ = hi_ + 1; st_ <<= 1; "
                  f"hi_ = j{u} + st_; }}",
                  f"{ind}    if (hi_ > a1_{u}) hi_ = a1_{u};",
                  f"{ind}  }}",
                  f"{ind}  while (lo_ < hi_) {{ const {IX} md_ = (lo_ + hi_) >> 1; "
                  f"if (IMG(md_) < key_) lo_ = md_ + 1; else hi_ = md_; }}",
                  f"{ind}  m{u} = lo_;",
                  f"{ind}  hit{u} = lo_ < a1_{u} && IMG(lo_) == key_;",
                  f"{ind}  const {IX} jm{u} = hit{u} ? lo_ : 0;"])
        gm = self.gen(f"jm{u}")
        for sl in f.stage_slots:
            J._uload(gm, sl, f"h{u}", b, ind + "  ")
        b.append(f"{ind}  tg{u} = {self.tag_expr(gm, f'h{u}', u)};")
        if f.pair:
            b.append(f"{ind}  tgb{u} = {self.lit_b(self.tag_expr(gm, f'h{u}', u))};")
        b.append(f"{ind}}}")
        if f.bounds:
            # a run whose bound fails a left conjunct holds no passing row
            ok = " && ".join(f"(bm{i}_{u} {cmp} hs_c20(a.{lit}) + 32768)"
                             for i, (_, lit, cmp) in enumerate(f.bounds))
            b.append(f"{ind}tg{u} = ({ok}) ? tg{u} : 0u;")
            if f.pair:
                b.append(f"{ind}tgb{u} = ({self.lit_b(ok)}) ? tgb{u} : 0u;")
        return b

    def stores(self, u: int, ind: str) -> List[str]:
        """The 2W tag words of 64-run group ``gi + u`` from the lanes' tags ``tg<u>`` (pair: and
        ``tgb<u>`` into ``tags_b``): whole words, plain stores; and the recorded match."""
        f, W, b = self.f, self.f.W, []  # noqa: N806
        if W == 1:
            for tg, tags in (("tg", "tags"), ("tgb", "tags" + PAIR_SFX))[:2 if f.pair else 1]:
                b.extend([f"{ind}{{ const u64 bal_ = __ballot({tg}{u} != 0u);",
                          f"{ind}  if (in{u} && lane < 2) a.{tags}[((gi + {u}) << 1) + lane] = "
                          f"(unsigned)(bal_ >> (32 * lane)); }}"])
        else:
            per_w = 32 // W
            b.extend([f"{ind}{{ unsigned wd_ = 0u;",
                      f"{ind}  for (int i_ = 0; i_ < {per_w}; ++i_) {{",
                      f"{ind}    const int src_ = ((lane * {per_w}) + i_) & 63;",
                      f"{ind}    wd_ |= (((unsigned)__shfl((int)tg{u}, src_, 64)) & {f.MASK}u) << "
                      f"(unsigned)(i_ * {W}); }}",
                      f"{ind}  if (in{u} && lane < {2 * W}) a.tags[(gi + {u}) * {2 * W} + lane] = "
                      f"wd_; }}"])
        if f.rec:
            b.append(f"{ind}if (in{u} && r{u} < a.NRUNS) a.MOUT[r{u}] = hit{u} ? (int)m{u} : -1;")
        return b

    def iteration(self, fast: bool, ind: str) -> List[str]:
        """U groups: all loads, then the resolves and stores, then the next iteration's guess."""
        U, IX, b = self.f.U, self.f.IX, []  # noqa: N806
        for u in range(U):
            b += self.group(u, fast, ind)
        for u in range(U):
            b += self.resolve(u, ind, self.f.lo16 and fast) + self.stores(u, ind)
        # next iteration's guess: the last group's last lane, when it matched in this range
        return b + [f"{ind}{{ const {IX} nx_ = __shfl((hit{U - 1} && own{U - 1}) ? m{U - 1} + 1 : "
                    f"({IX})-1, 63, 64);",
                    f"{ind}  gbase = nx_; }}"]

    def group_loop(self) -> List[str]:
        """The one-run-per-lane kernel's loop: RT2_UNROLL groups in flight per iteration."""
        U = self.f.U  # noqa: N806
        return [f"  for (i64 gi = gbeg; gi < gend; gi += {U}) {{"] + \
            self.advance("(gi << 6)", "    ", True) + [
            # wavefront-uniform: every run of this iteration's groups belongs to range rg (or none)
            f"    if (((gi + {U}) << 6) <= nxt0) {{"] + self.iteration(True, "      ") + [
            "    } else {   // a range starts inside this iteration's groups"] + \
            self.iteration(False, "      ") + ["    }", "  }"]

    def vec_types(self) -> List[str]:
        """4 consecutive elements at an element-aligned address (the guess is arbitrary): one
        load."""
        f, g = self.f, self.gen("row_")
        rkt = g.raw_type(self.rk)
        b = ["typedef int hs_i4 __attribute__((ext_vector_type(4)));"] + \
            (["typedef unsigned short hs_us4 __attribute__((ext_vector_type(4)));"]
             if f.bounds or f.k16 else []) + \
            (["typedef unsigned short hs_ro4 __attribute__((ext_vector_type(4), aligned(2)));"]
             if f.k16 else []) + [
                f"typedef {rkt} hs_rk4 __attribute__((ext_vector_type(4), "
                f"aligned({J._SIZEOF[rkt]})));"]
        for sl in f.stage_slots:
            t = g.raw_type(sl)
            b.append(f"typedef {t} hs_c{sl}x4 __attribute__((ext_vector_type(4), "
                     f"aligned({J._SIZEOF[t]})));")
        return b

    def stage_regs(self) -> List[str]:
        """The two register sets (A / B) of the pipeline, and ``slow_``."""
        f, b = self.f, []
        for s in ("A", "B"):
            b.append(f"  int pb{s} = 0; " + " ".join(
                (f"hs_us4 L{s}{u} = {{}}; hs_ro4 R{s}{u} = {{}}; int LG{s}{u} = 0, RG{s}{u} = 0, "
                 f"RH{s}{u} = 0;" if f.k16 else f"hs_v4u L{s}{u} = {{}}; hs_rk4 R{s}{u} = {{}};") +
                "".join(f" hs_us4 M{i}{s}{u} = {{}};" for i in range(len(f.bounds))) +
                "".join(f" hs_c{sl}x4 C{sl}{s}{u} = {{}};" for sl in f.stage_slots)
                for u in range(f.U)))
        if f.k16:
            # blocks still to take the 64-run code after a stage met a wide group
            b.append("  int slow_ = 0;")
        return b

    def fast(self, blk: str, off: int, ind: str) -> List[str]:
        """``f_``: the stage of blocks blk .. blk + U - 1 is fast at guess base ``base_`` (the
        resolved base + ``off``, or range-relative) - all wavefront-uniform, tested before any
        address is formed."""
        U, R = self.f.U, 256 * self.f.U  # noqa: N806
        return [f"{ind}const int rb_ = ({blk}) << 8;",
                f"{ind}const int base_ = gbase >= 0 ? gbase + {off} : s0 + (rb_ - lr0);",
                f"{ind}const bool f_ = {'slow_ == 0 && ' if self.f.k16 else ''}({blk}) + {U} <= bend && "
                f"rb_ >= lr0 && "
                f"rb_ + {R} <= lr1 && rb_ + {R} <= NR && (i64)rb_ + {R} <= nxt0 && "
                f"base_ >= s0 && base_ + {R} <= s1;"]

    def load(self, s: str, run0: str, base: str, ind: str) -> List[str]:
        """Set ``s`` <- the stage whose first run is ``run0`` (a multiple of 256), guessed at
        right row ``base``; the caller has tested both (``fast``).  Per block one 16-byte load
        of the lane's 4 left keys, one element-aligned 4-element load of the right key and of
        each staged right column at the guess, and one 8-byte load of its runs' bounds.

        ``k16``: both key columns come as uint16 offsets (``LO16`` per run, ``RO16`` per right
        row: one 8-byte load each per lane and block) plus the bases of their 32-element groups
        (``LG16`` / ``RG16``: one dword for the lane's four runs, two for its four right rows,
        which can straddle one group edge; the group index comes from the run / guessed row, so
        nothing depends on a load) - 8.25 instead of 12 B per run with one bound."""
        f, g, b = self.f, self.gen("row_"), [f"{ind}pb{s} = {base};"]
        for u in range(f.U):
            if f.k16:
                lr_, rr_ = f"({run0} + {256 * u} + 4 * lane)", f"({base} + {256 * u} + 4 * lane)"
                b.extend([f"{ind}L{s}{u} = *(const hs_us4*)(a.LO16 + {lr_});",
                          f"{ind}R{s}{u} = *(const hs_ro4*)(a.RO16 + {rr_});",
                          f"{ind}LG{s}{u} = a.LG16[{lr_} >> 5];",
                          f"{ind}RG{s}{u} = a.RG16[{rr_} >> 5]; "
                          f"RH{s}{u} = a.RG16[({rr_} + 3) >> 5];"])
            else:
                b.extend([f"{ind}L{s}{u} = *(const hs_v4u*)(a.RK{self.lk} + ({run0} + {256 * u} + "
                          f"4 * lane));",
                          f"{ind}R{s}{u} = *(const hs_rk4*)({g.ptr(self.rk)} + ({base} + {256 * u} + "
                          f"4 * lane));"])
            for i, (arr, _, _) in enumerate(f.bounds):
                b.append(f"{ind}M{i}{s}{u} = *(const hs_us4*)(a.{arr} + ({run0} + {256 * u} + "
                         f"4 * lane));")
            for sl in f.stage_slots:
                b.append(f"{ind}C{sl}{s}{u} = *(const hs_c{sl}x4*)({g.ptr(sl)} + "
                         f"({base} + {256 * u} + 4 * lane));")
        return b

    def resolve_stage(self, s: str, ind: str) -> List[str]:
        """Tags (and matches) of the stage in register set ``s``: blocks nb .. nb + U - 1,
        loaded at guess base pb<s>; four compares per lane and block, a miss gallops per run
        through ``resolve``; leaves the resolved next base in ``gbase``.  Compare, key frame,
        miss path and tags are the same with ``k16``, which rebuilds code = base + offset."""
        f, W, L, g = self.f, self.f.W, self.f.L, self.gen("row_")  # noqa: N806
        b = [f"{ind}int nx_ = -1;"]
        for u in range(f.U):
            b.append(f"{ind}{{ unsigned pk_ = 0u;" + (" unsigned pkb_ = 0u;" if f.pair else "") +
                     (" hs_i4 mo_;" if f.rec else ""))
            i2 = ind + "  "
            for k in range(4):
                x = f"{s}{u}_{k}"
                b.extend([f"{i2}{{ const int j{x} = pb{s} + {256 * u + k} + 4 * lane;",
                          f"{i2}const int a0_{x} = s0, a1_{x} = s1; const bool act{x} = true;"])
                if f.k16:
                    # code = group base + offset (exact); right row k is in the group of the
                    # lane's first row or, past a group edge, of its last
                    b.extend([f"{i2}const unsigned key{x} = (unsigned)LG{s}{u} + "
                              f"(unsigned)L{s}{u}[{k}] + (unsigned)a.KOF;",
                              f"{i2}const unsigned k{x} = IMGV((int)((unsigned)"
                              f"((((pb{s} + {256 * u} + 4 * lane) & 31) + {k}) < 32"
                              f" ? RG{s}{u} : RH{s}{u}) + (unsigned)R{s}{u}[{k}]));"])
                else:
                    b.extend([f"{i2}const unsigned key{x} = L{s}{u}[{k}] + (unsigned)a.KOF;",
                              f"{i2}const unsigned k{x} = IMGV(R{s}{u}[{k}]);"])
                for i in range(len(f.bounds)):
                    b.append(f"{i2}const int bm{i}_{x} = (int)M{i}{s}{u}[{k}];")
                for sl in f.stage_slots:
                    J._uload_raw(g, sl, f"g{x}", f"C{sl}{s}{u}[{k}]", "1", b, i2)
                b += self.resolve(x, i2)
                b.append(f"{i2}pk_ |= (tg{x} & {f.MASK}u) << {k * W};")
                if f.pair:
                    b.append(f"{i2}pkb_ |= (tgb{x} & {f.MASK}u) << {k * W};")
                if f.rec:
                    b.append(f"{i2}mo_[{k}] = hit{x} ? m{x} : -1;")
                if u == f.U - 1 and k == 3:
                    b.append(f"{i2}nx_ = hit{x} ? m{x} + 1 : -1;")
                b.append(f"{i2}}}")
            # the lanes of one tag word hold disjoint bit fields: OR across them, one stores
            for pk, tags in (("pk_", "tags"), ("pkb_", "tags" + PAIR_SFX))[:2 if f.pair else 1]:
                if L > 1:
                    b.append(f"{i2}{pk} <<= (unsigned)({4 * W} * (lane & {L - 1}));")
                o = 1
                while o < L:
                    b.append(f"{i2}{pk} |= (unsigned)__shfl_xor((int){pk}, {o}, 64);")
                    o <<= 1
                b.append(f"{i2}if ((lane & {L - 1}) == 0) a.{tags}[(nb + {u}) * {8 * W} + "
                         f"(lane >> {L.bit_length() - 1})] = {pk};")
            if f.rec:
                b.append(f"{i2}*(hs_i4*)(a.MOUT + (((nb + {u}) << 8) + 4 * lane)) = mo_;")
            b.append(f"{ind}}}")
        return b + [f"{ind}gbase = __builtin_amdgcn_readlane(nx_, 63);"]

    def slow_block(self) -> List[str]:
        """Block nb through the 64-run ``group`` / ``resolve``, one group at a time, on the
        32-bit arrays."""
        return ["    if (!f_) {   // slow block: its 64-run groups one at a time",
                "#pragma unroll 1",
                "      for (i64 gi = (i64)nb << 2; gi < (((i64)nb + 1) << 2) && gi < gend; ++gi) {"] + \
            self.advance("(gi << 6)", "        ") + self.group(0, False, "        ") + \
            self.resolve(0, "        ") + self.stores(0, "        ") + [
                "        gbase = __builtin_amdgcn_readlane((hit0 && own0) ? m0 + 1 : -1, 63);",
                "      }"] + (["      slow_ -= slow_ > 0 ? 1 : 0;"] if self.f.k16 else []) + [
                "      ++nb; continue;",
                "    }"]

    def pipeline(self) -> List[str]:
        """The fast stages from nb on.  The guess of the stage after the current one assumes
        every run matches (current base + its runs), so its loads are issued before the current
        stage is resolved - two register sets, the loop unrolled by two so neither is copied;
        the resolved base (last match + 1) replaces the assumption for the stage after that."""
        f, U, R = self.f, self.f.U, 256 * self.f.U  # noqa: N806
        b = self.load("A", "rb_", "base_", "    ") + ["    for (;;) {"]
        for s, t in (("A", "B"), ("B", "A")):
            # set s holds the stage at nb: issue the next stage's loads into set t, then resolve s.
            # The loads are unconditional (under a branch the compiler would wait for them where
            # the paths merge): when the next stage is not fast they re-read this stage's
            # addresses, which passed the test, and the loop ends after this stage
            b += ["      {"] + self.fast(f"nb + {U}", R, "        ") + [
                f"        const int nr_ = f_ ? rb_ : (nb << 8), nj_ = f_ ? base_ : pb{s};"] + \
                self.load(t, "nr_", "nj_", "        ")
            if f.k16:
                # a wide group (``WIDE_GROUP``) among this stage's loaded bases (a ballot after the
                # loads; wavefront-uniform): its blocks take the 64-run code on the 32-bit arrays,
                # as the gallop always does (nb and gbase still name this stage)
                wd = " || ".join(f"{r}{s}{u} == (int)0x80000000" for u in range(U)
                                 for r in ("LG", "RG", "RH"))
                b.append(f"        if (__ballot({wd}) != 0ull) {{ slow_ = {U}; "
                         "__builtin_amdgcn_s_waitcnt(0x0F70); break; }")
            b += self.resolve_stage(s, "        ")
            # (leaving the loop: drain the re-read, or the compiler's wait counts, which merge
            # every path into the loop head, would wait for it in every iteration: vmcnt(0))
            b += [f"        nb += {U};",
                  "        if (!f_) { __builtin_amdgcn_s_waitcnt(0x0F70); break; }",
                  "      }"]
        return b + ["    }"]

    def block_loop(self) -> List[str]:
        """The four-runs-per-lane kernel's loop (``tags2_wide``): the chunk is counted in 256-run
        blocks, lane l owning runs 256 b + 4 l .. + 3.  A block whose runs all lie in one range
        and below NRUNS, and whose 256 guessed right rows lie in [s0, s1), is *fast*; every other
        block (a range edge, the table tail, a guess outside the bucket) is a ``slow_block``."""
        return self.stage_regs() + ["  int nb = bbeg;", "  while (nb < bend) {"] + \
            self.advance("((i64)nb << 8)", "    ") + self.fast("nb", 0, "    ") + \
            self.slow_block() + self.pipeline() + ["  }"]

    def recorded_loop(self) -> List[str]:
        """Phase 1 over a recorded match (``match``): per run one int32 load of its right row
        (-1: no match, or the run is outside the lowering's ranges), then the right predicate /
        group columns at that row.  No key images, no range table, no gallop: the record already
        resolved them (``record_matches``: it depends only on the lowering's ranges and the key
        columns, not on the literals), so the phase reads 4 bytes per run plus the staged right
        columns (monotone rows: coalesced).

        ``copy``: the right columns were gathered into run order at the record (``S<slot>`` /
        ``SV<slot>``, ``gen_match_gather``; added here at the first group's loads) and the match
        is one bit per run (``HIT``, one 64-bit word per 64-run group, read once per wavefront):
        the phase reads the stored codes of its predicate columns per run and nothing at right
        rows."""
        f, args, cols, ind = self.f, self.args, self.cols, "    "
        b = [f"  for (i64 gi = gbeg; gi < gend; gi += {f.U}) {{"]
        for u in range(f.U):
            # the record is padded to whole groups: an in-range group's 64 lanes all read it
            b.append(f"{ind}const bool in{u} = gi + {u} < gend;")
            if f.copy:
                b.extend([f"{ind}const int r{u} = in{u} ? (int)(((gi + {u}) << 6) + lane) : lane;",
                          f"{ind}const u64 hb{u} = a.HIT[in{u} ? gi + {u} : 0];"])
                for sl in f.stage_slots:
                    t = self.gen("r_").raw_type(sl)
                    sp = args.add("p", f"S{sl}", f"const {t}*")
                    b.append(f"{ind}const {t} w{sl}_g{u} = {sp}[r{u}];")
                    if cols[sl][1]:
                        vp = args.add("p", f"SV{sl}", "const unsigned char*")
                        b.append(f"{ind}const unsigned char u{sl}_g{u} = {vp}[r{u}];")
            else:
                b.append(f"{ind}const int mt{u} = a.MATCH[in{u} ? (((gi + {u}) << 6) + lane) : lane];")
        for u in range(f.U):
            if f.copy:
                b.append(f"{ind}const bool hit{u} = in{u} && ((hb{u} >> lane) & 1ull);")
                gu = self.gen(f"r{u}")
                for sl in f.stage_slots:
                    J._uload_raw(gu, sl, f"g{u}", f"w{sl}_g{u}", f"u{sl}_g{u}", b, ind)
                continue
            b.extend([f"{ind}const bool hit{u} = in{u} && mt{u} >= 0;",
                      f"{ind}const int j{u} = hit{u} ? mt{u} : 0;"])
            gu = self.gen(f"j{u}")
            for sl in f.stage_slots:
                J._uload(gu, sl, f"g{u}", b, ind)
        for u in range(f.U):
            b.append(f"{ind}const unsigned tg{u} = {self.tag_expr(self.gen(f'j{u}'), f'g{u}', u)};")
            b += self.stores(u, ind)
        return b + ["  }"]


def gen_run_tags2(p: NL.JoinParams, compacts, W: int, ix32: bool = False,
                  mode: str = "", prune: tuple = (), k16: bool = False,
                  pair: bool = False) -> J.Kernel:
    """Phase 1, direct form (``_Tags2``).  The forms (``_tags_form``) and their stages:

    * mode "" / "rec" (also stores each run's matched right row, or -1, into ``MOUT``) / "lo16",
      one run per lane: ``group_loop`` - per iteration U ``group`` loads, then ``resolve`` and
      ``stores`` per group;
    * the same modes, four runs per lane (``tags2_wide``): ``block_loop`` - ``fast`` test, then
      ``slow_block`` or the ``pipeline`` of ``load`` and ``resolve_stage``; with ``prune``
      (``prune_plan``) bounds, ``k16`` (``tags2_k16``) key offsets and for a ``pair``
      (``tags2_pair``: every tag word stored twice, the second query's into ``tags_b``; each
      bitmap is what the single kernel writes for that literal set);
    * "match" / "copy": ``recorded_loop`` over ``MATCH`` (one int32 per run, -1 padded to whole
      64-run groups) or ``HIT`` and the column copies, instead of the run keys, the key images
      and the range table;
    * "lo16prep" (kernel ``hs_jit_key_lo16``): ``prep_body``.

    The driver is the kernel top to bottom; its order is also the order in which argument slots
    are added (``_Tags2``), so it is part of the sources' text."""
    s = _Tags2(p, compacts, W, ix32, mode, prune, k16, pair)
    s.header()
    if s.f.match or s.f.copy:
        b = s.prologue() + s.recorded_loop()
    elif s.f.prep:
        b = s.images() + s.prep_body()
    else:
        b = s.images() + s.prologue() + s.seek() + \
            (s.block_loop() if s.f.wide == 4 else s.group_loop())
    return J._kernel(s.f.name, s.args, b, tdefs=s.vec_types() if s.f.wide == 4 else ())


def copy_ok(p: NL.JoinParams, compacts) -> bool:
    """Whether phase 1 can read per-run copies of its right columns (mode "copy"): every staged
    column is stored plainly or as a one-array compact code (not the grouped 16-bit form)."""
    cols = J._col_specs(p, compacts)
    for sl in _stage_slots(p):
        enc = cols[sl][2]
        if enc and len(enc) > 2 and enc[2] == 64:
            return False
    return True


def record_matches(p: NL.JoinParams, compacts, W: int, vt: dict, nruns: int, grid: int, dev):
    """Each run's matched right row under the lowering's ranges (or -1), padded with -1 to whole
    64-run groups: one launch of the verifying phase 1 in mode "rec" at lowering time (queued on
    the current stream).  Literal-independent: the ranges, key frame and key columns are fixed
    for the launcher, and the record mode stores the match before any right predicate."""
    import torch
    m = torch.full((((nruns + 63) >> 6) * 64,), -1, dtype=torch.int32, device=dev)
    kr = J.kernel_for(tags2_shape(p, compacts, W, True, "rec"),
                      lambda: gen_run_tags2(p, compacts, W, True, "rec"))
    v = dict(vt)
    v["MOUT"] = m.data_ptr()
    J.fill_preds_aggs(v, [(k_, p.preds[k_]) for k_ in range(p.npreds)], [], compacts)
    kr.launch(grid, v, NL.stream_ptr(), 0)
    return m


def gen_match_gather(p: NL.JoinParams, compacts) -> J.Kernel:
    """The right columns phase 1 reads, gathered into run order at the recorded match
    (``S<slot>`` stored elements, ``SV<slot>`` validity bytes; row 0 for a run without one - its
    HIT bit is clear): one pass at record time for the "copy" form of phase 1."""
    args = J.Args()
    args.add("p", "MATCH", "const int*")
    args.add("q", "N", "long long")
    cols = J._col_specs(p, compacts)
    g = J._Gen(args, cols, SPLIT, ("j_", "j_"), frozenset(), True)
    b = [f"  for (i64 i = (i64)blockIdx.x * {J.BLOCK} + threadIdx.x; i < a.N; "
         f"i += (i64)gridDim.x * {J.BLOCK}) {{",
         "    const int m_ = a.MATCH[i]; const int j_ = m_ >= 0 ? m_ : 0;"]
    for sl in _stage_slots(p):
        sp = args.add("p", f"S{sl}", f"{g.raw_type(sl)}*")
        b.append(f"    {sp}[i] = {g.ptr(sl)}[j_];")
        if cols[sl][1]:
            vp = args.add("p", f"SV{sl}", "unsigned char*")
            b.append(f"    {vp}[i] = {g.vptr(sl)}[j_];")
    b.append("  }")
    return J._kernel("hs_jit_match_gather", args, b)


def copy_matches(p: NL.JoinParams, compacts, m, vt: dict, dev) -> tuple:
    """From a recorded match ``m``: the HIT words (bit l of word g: run 64 g + l has a right
    row) and the gathered right columns; returns (tensors to keep, their argument values)."""
    import torch
    n = int(m.numel())
    hit = ((m.view(-1, 64) >= 0).to(torch.int64) <<
           torch.arange(64, device=dev, dtype=torch.int64)).sum(1)  # distinct bits: sum == OR
    keep, vals = [hit], {"HIT": hit.data_ptr()}
    cols = J._col_specs(p, compacts)
    g = J._Gen(J.Args(), cols, SPLIT, ("j_", "j_"), frozenset(), True)
    for sl in _stage_slots(p):
        t = torch.empty(n * J._SIZEOF[g.raw_type(sl)], dtype=torch.uint8, device=dev)
        keep.append(t)
        vals[f"S{sl}"] = t.data_ptr()
        if cols[sl][1]:
            v = torch.empty(n, dtype=torch.uint8, device=dev)
            keep.append(v)
            vals[f"SV{sl}"] = v.data_ptr()
    kg = J.kernel_for(("match_gather", tags2_shape(p, compacts, 1)[1], tuple(_stage_slots(p)),
                       J.BLOCK),
                      lambda: gen_match_gather(p, compacts))
    a = dict(vt, MATCH=m.data_ptr(), N=n, **vals)
    kg.launch(max(1, min(8192, (n + J.BLOCK - 1) // J.BLOCK)), a, NL.stream_ptr(), 0)
    return keep, vals


def lo16_keys(p: NL.JoinParams, compacts, W: int, vt: dict, nruns: int, nright: int, grid: int,
              dev):
    """The low 16 bits of the left run key images and the right key images (phase 1's checked
    groups compare these: ``gen_run_tags2`` mode "lo16"), computed once per reused lowering;
    None when the right key has nulls (a null's image 0 could alias a left key's low half).
    Literal-independent encodings of the key columns: every query still matches its keys."""
    import torch
    from .device_cache import track_derived
    if J._col_specs(p, compacts)[p.rkey][1]:
        return None
    ll = torch.empty(max(nruns, 1), dtype=torch.int16, device=dev)
    rl = torch.empty(max(nright, 1), dtype=torch.int16, device=dev)
    kp = J.kernel_for(tags2_shape(p, compacts, W, True, "lo16prep"),
                      lambda: gen_run_tags2(p, compacts, W, True, "lo16prep"))
    kp.launch(grid, dict(vt, LL=ll.data_ptr(), RL=rl.data_ptr(), NRIGHT=nright),
              NL.stream_ptr(), 0)
    track_derived(ll)
    track_derived(rl)
    return ll, rl


def run_ranges(rstart, rlen, rbucket, roff, runs):
    """RNG of ``gen_run_tags2``: per non-empty left row range (first run, end run, right bucket
    rows [s0, s1)), sorted by first run; computed once per lowering (one small D2H)."""
    import numpy as np
    import torch
    rs = rstart.cpu().numpy().astype(np.int64)
    rl = rlen.cpu().numpy().astype(np.int64)
    rb = rbucket.cpu().numpy().astype(np.int64)
    ro = roff.cpu().numpy().astype(np.int64)
    keep = rl > 0
    rs, rl, rb = rs[keep], rl[keep], rb[keep]
    if len(rs) == 0:
        return np.zeros((0, 4), np.int64)
    rows = np.concatenate([rs, rs + rl - 1])
    gi = torch.from_numpy(rows >> 6).to(runs.gmask.device)
    gm = runs.gmask.index_select(0, gi).cpu().numpy().view(np.uint64)
    gr = runs.gruns.index_select(0, gi).cpu().numpy().astype(np.int64)
    full = (1 << 64) - 1
    # run of a row: the group's first run + run starts among the group's rows 1..i
    run = np.array([int(g_) + bin(int(m_) & (((2 << int(r_ & 63)) - 2) & full)).count("1")
                    for g_, m_, r_ in zip(gr, gm, rows)], dtype=np.int64)
    n = len(rs)
    out = np.stack([run[:n], run[n:] + 1, ro[rb], ro[rb + 1]], axis=1)
    return out[np.argsort(out[:, 0], kind="stable")]


def scan_shape(p: NL.JoinParams, compacts, W: int, NI: int) -> tuple:
    cols = tuple(sorted((s, c) for s, c in J._col_specs(p, compacts).items() if s < SPLIT))
    preds = J._preds_shape(p, 0, p.nlp)
    aggs = tuple((p.aggs[i].kind, p.aggs[i].nterms, tuple(p.aggs[i].col[:p.aggs[i].nterms]))
                 for i in range(p.naggs))
    return ("run_scan", cols, preds, aggs, p.group_col, p.lkey, W, NI, J.BLOCK, J.WAVE_SYNC,
            J.VEC_PREFETCH, _scan_grouped(p))


def _scan_grouped(p: NL.JoinParams) -> bool:
    """Whether the scan phase keeps a group table: a right-side group key with a single group
    (a constant column) accumulates like an ungrouped aggregate (same partials layout)."""
    return p.group_col >= 0 and not (p.group_col >= SPLIT and p.num_groups == 1)


def gen_run_scan(p: NL.JoinParams, compacts, W: int, NI: int) -> J.Kernel:
    """Phase 2 (module docstring): the left rows' scan with the run-tag test."""
    args, lk = _scan_args(p), p.lkey
    cols = J._col_specs(p, compacts)
    lpreds = _lpreds(p)
    aggs = J.aggs_of(p)
    grouped = _scan_grouped(p)
    rgroup = grouped and p.group_col >= SPLIT
    pslots = J._pred_slots(lpreds)
    tail = J._agg_slots(aggs) + ([p.group_col] if grouped and not rgroup else [])
    allslots = list(dict.fromkeys(pslots + tail))
    approx = J._sum_only_slots(lpreds, aggs, p.group_col if grouped and not rgroup else -1, cols)
    MASK = (1 << W) - 1  # noqa: N806
    KW = ((31 + (NI - 1) * W) >> 5) + 1  # noqa: N806 — tag words a thread's rows can touch
    st = J._Stream(args, cols, SPLIT, approx, NI)
    ind = st.ind
    g1 = st.gen("row0")
    b: List[str] = []
    b += J._acc_decls(aggs, grouped, args)

    def body(b: List[str], full: bool) -> None:
        J._vec_load_slots(b, g1, pslots, NI, ind)
        for it in range(NI):
            b.append(f"{ind}bool pass{it} = act{it} && "
                     f"{J._rename(st.gen(f'row{it}').cnf(lpreds), allslots, it)};")
        # row -> run: the thread's NI rows lie in one 64-row group (NI | 64, g0 % NI == 0)
        b += [f"{ind}const int sh_ = (int)(g0 & 63);",
              f"{ind}const i64 r0_ = (i64)gr_ + (i64)__popcll(gm_ & ((2ull << sh_) - 2ull));",
              f"{ind}const unsigned gl_ = (unsigned)(gm_ >> sh_);",
              f"{ind}const i64 b0_ = r0_ * {W};",
              f"{ind}const i64 w0_ = b0_ >> 5;",
              f"{ind}" + " ".join(f"const unsigned tw{k}_ = a.tags[w0_ + {k}];" for k in range(KW))]
        for it in range(NI):
            ri = "0" if it == 0 else f"(int)__popc(gl_ & {(2 << it) - 2}u)"
            b.append(f"{ind}{{ const int rel = (int)(b0_ & 31) + {ri} * {W};")
            sel = f"tw{KW - 1}_"
            for k in reversed(range(KW - 1)):
                sel = f"((rel >> 5) == {k} ? tw{k}_ : {sel})"
            b += [f"{ind}  const unsigned tg = ({sel} >> (unsigned)(rel & 31)) & {MASK}u;",
                  f"{ind}  pass{it} = pass{it} && tg != 0u;",
                  f"{ind}  jg{it} = (int)tg - 1; }}"]
        b.extend(J._compacted_tail(st, aggs, p.group_col if grouped else -1, allslots,
                                   J._Tail(with_j=rgroup, j_fmt="jg{it}", jgroup=rgroup)))

    def body_decl(b: List[str], full: bool) -> None:
        b.append(f"{ind}int " + ", ".join(f"jg{it} = 0" for it in range(NI)) + ";")
        body(b, full)

    gi = "((G0 < a.nrows ? G0 : a.nrows - 1) >> 6)"
    J._vec_tiles(st, b, body_decl, J._Tile(
        J._vec_loads(g1, pslots),
        [("gm_", "unsigned long long", f"a.GM{lk}[{gi}]"), ("gr_", "int", f"a.GR{lk}[{gi}]")]))
    b += ["  }"]
    b += J._flush(aggs, grouped)
    Wv = J.BLOCK // 64  # noqa: N806
    st.lds += [f"  typedef {J._crow_t(st.T)} crow_t; __shared__ crow_t crow_s[{Wv}][{64 * NI}];",
               "  const int cln = threadIdx.x & 63, wv = threadIdx.x >> 6;"]
    if rgroup:
        st.lds.append(f"  __shared__ int cj_s[{Wv}][{64 * NI}];")
    return st.finish("hs_jit_run_scan", b, (len(aggs) * p.num_groups * 32) if grouped else 0)


# phase 2 for 1-bit tags: masks 64 rows at a time (gen_run_sparse_scan; RS_BITS), aggregate
# inputs read row-packed when they fit one 64-bit word (pack_layout / packed_tail; RS_PACK).  (A
# row-mask expansion between the phases with a gated dense scan measured no faster: removed.)


def _tail_slots(p: NL.JoinParams) -> list:
    grouped = _scan_grouped(p)
    aggs = J.aggs_of(p)
    return list(dict.fromkeys(J._agg_slots(aggs) + ([p.group_col] if grouped else [])))


def pack_layout(p: NL.JoinParams, compacts, extra: tuple = ()) -> Optional[tuple]:
    """((slot, bit offset, code bytes), ...) of the row-packed aggregate inputs of the bits
    scan: two or more compact-coded tail columns without validity whose codes fit 64 bits.
    ``extra``: the predicate columns the candidate form of phase 2 tests on the word
    (``prune_plan``), as further fields after the aggregate inputs (their full codes)."""
    if not RS_PACK:
        return None
    slots = list(dict.fromkeys(_tail_slots(p) + list(extra)))
    if len(slots) < 2:
        return None
    out, off = [], 0
    for sl in slots:
        c = (compacts or {}).get(sl)
        if c is None or p.cols[sl].valid or getattr(c, "runs", None) or \
                type(c).__name__ != "Compact" or c.width not in (1, 2, 4):
            return None
        out.append((sl, off, c.width))
        off += 8 * c.width
    return tuple(out) if off <= 64 else None


# (ids of the packed code tensors) -> (the tensors, packed int64 words): derived per resident
# table once, like the compact codes themselves
_PACKS: dict = {}


def packed_tail(layout, compacts):
    """One int64 word per row: each layout column's code at its bit offset (uint bits)."""
    import torch
    key = tuple(id(compacts[sl].codes) for sl, _, _ in layout)
    hit = _PACKS.get(key)
    if hit is not None and all(a is compacts[sl].codes for a, (sl, _, _) in zip(hit[0], layout)):
        return hit[1]
    n = compacts[layout[0][0]].codes.numel()
    w = torch.zeros(n, dtype=torch.int64, device=compacts[layout[0][0]].codes.device)
    for sl, off, nb in layout:
        c = compacts[sl].codes.to(torch.int64) & ((1 << (8 * nb)) - 1)
        w |= c << off
        del c
    if len(_PACKS) >= 8:
        _PACKS.pop(next(iter(_PACKS)))
    _PACKS[key] = (tuple(compacts[sl].codes for sl, _, _ in layout), w)
    return w


# 12-bit packed copies of 16-bit predicate codes (the bits scan's row stream): 64 rows in 24
# dwords, 8 rows per 3 dwords (value j at bits [12 j, 12 j + 12) of the 96-bit chunk) - 25% fewer
# bytes for the one column phase 2 reads for every row.  Derived once per resident table (like
# the compact codes and the row-packed aggregate inputs), kept while its codes are.
_P12: dict = {}


# per-run bounds of a left predicate column over the join key's run form (``prune_plan``):
# (id of the codes, id of the run masks) -> (those tensors, min, max).  Derived once per resident
# table and column, like the packed copies above; they depend on no literal.
_RBOUNDS: dict = {}


def run_bounds(runs, c) -> tuple:
    """(mn, mx) of 16-bit compact column ``c`` per run of ``runs`` (a RunCompact of the same
    table): uint16 bits of code + 32768, padded to whole 256-run blocks with the empty interval
    (``ops.kernels.run_minmax16``)."""
    from ..ops import kernels as K
    from .device_cache import track_derived
    key = (id(c.codes), id(runs.gmask))
    hit = _RBOUNDS.get(key)
    if hit is not None and hit[0] is c.codes and hit[1] is runs.gmask:
        return hit[2], hit[3]
    mn, mx = K.run_minmax16(runs.gmask, runs.gruns, runs.nruns, c.codes)
    track_derived(mn)
    track_derived(mx)
    if len(_RBOUNDS) >= 8:
        _RBOUNDS.pop(next(iter(_RBOUNDS)))
    _RBOUNDS[key] = (c.codes, runs.gmask, mn, mx)
    return mn, mx


def _p12_offset(c) -> int:
    """The smallest code of compact column ``c`` (codes = value - base, values in [lo, hi])."""
    return int(c.lo) - int(c.base)


def pack12_ok(c) -> bool:
    """Whether compact column ``c``'s codes are 16-bit and span at most 4096 values (host
    metadata): the packed copy stores code - (lo - base) in 12 bits."""
    if c is None or type(c).__name__ != "Compact" or c.width != 2 or getattr(c, "runs", None):
        return False
    if c.lo is None or c.hi is None:
        return False
    return 0 <= int(c.hi) - int(c.lo) <= 4095


def packed12(c):
    """The 12-bit packed copy of compact column ``c`` (``pack12_ok``), cached per codes tensor."""
    import torch
    key = id(c.codes)
    hit = _P12.get(key)
    if hit is not None and hit[0] is c.codes:
        return hit[1]
    n = c.codes.numel()
    npad = (n + 63) // 64 * 64
    v = torch.zeros(npad, dtype=torch.int64, device=c.codes.device)
    v[:n] = (c.codes.to(torch.int64) - _p12_offset(c)) & 0xFFF
    v = v.view(-1, 8)
    a = v[:, 0] | (v[:, 1] << 12) | ((v[:, 2] & 0xFF) << 24)
    b = (v[:, 2] >> 8) | (v[:, 3] << 4) | (v[:, 4] << 16) | ((v[:, 5] & 0xF) << 28)
    cc = (v[:, 5] >> 4) | (v[:, 6] << 8) | (v[:, 7] << 20)
    w = torch.stack([a, b, cc], dim=1).reshape(-1)
    w = torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32).contiguous()
    del v, a, b, cc
    if len(_P12) >= 8:
        _P12.pop(next(iter(_P12)))
    _P12[key] = (c.codes, w)
    return w


def _p12_slots(p: NL.JoinParams, compacts) -> tuple:
    """Predicate slots of phase 2 that read a 12-bit packed copy (RS_PACK12), or ()."""
    if not RS_PACK12 or not RS_PK16:
        return ()
    slots = J._pred_slots(_lpreds(p))
    if not slots or any(p.cols[sl].valid or not pack12_ok((compacts or {}).get(sl))
                        for sl in slots):
        return ()
    # every leaf must have the packed range-test form (Gen.cnf_sign2)
    for _, pr in _lpreds(p):
        if pr.kind == NL.PK_TRUE:
            continue
        c = (compacts or {}).get(pr.col)
        scaled = c is not None and c.scale is not None
        if pr.col not in slots or pr.kind not in (NL.PK_INT_LIT, NL.PK_FLT_LIT, NL.PK_IS_NULL,
                                                   NL.PK_NOT_NULL):
            return ()
        if (pr.kind == NL.PK_INT_LIT and scaled) or (pr.kind == NL.PK_FLT_LIT and not scaled):
            return ()
    return tuple(slots)


def fill_pack12(vs: dict, p: NL.JoinParams, compacts) -> list:
    """The packed copies' pointers into a phase-2 argument dict; returns the tensors to keep."""
    keep = []
    for sl in _p12_slots(p, compacts):
        w = packed12(compacts[sl])
        vs[f"P12_{sl}"] = w.data_ptr()
        vs[f"P12O_{sl}"] = _p12_offset(compacts[sl])
        keep.append(w)
    return keep


def cand_pair(p: NL.JoinParams, compacts, cand: tuple, hk=None, tk=None) -> bool:
    """Whether the candidate phase 2 of this join has the pair form (RS_PAIR; kernel
    ``hs_jit_run_bits_cand2``): one pass gathers the tail words of two queries' candidates once.
    Only the headline's form: the candidate form (``cand`` from ``prune_plan``: plain
    aggregates in registers, no hash or top-K walk) with the nibble table (RS_LUT)."""
    return bool(RS_PAIR and RS_LUT and cand and hk is None and tk is None and
                not _scan_grouped(p) and pack_layout(p, compacts, cand) is not None)


def sparse_shape(p: NL.JoinParams, compacts, hk=None, tk=None, cand: tuple = (),
                 pair: bool = False) -> tuple:
    if cand:
        pair = bool(pair) and cand_pair(p, compacts, cand, hk, tk)
        return ("run_bits_cand2" if pair else "run_bits_cand", RS_WALK, RS_LUT, RS_WAVES,
                bool(RS_KEEP)) + scan_shape(p, compacts, 1, 64)[1:] + (pack_layout(p, compacts, cand),)
    return ("run_bits_scan", RS_PIPE, RS_WALK, RS_LDS, RS_LUT, RS_PK16, RS_WAVES,
            _p12_slots(p, compacts)) + scan_shape(p, compacts, 1, 64)[1:] + \
        (pack_layout(p, compacts),) + ((hk.shape(),) if hk is not None else ()) + \
        ((tk.shape(),) if tk is not None else ())


# the bit-parallel phase 2: rows per wavefront tile (64 groups, one per lane) and list entries per
# wavefront and round (a denser tile takes rounds)
BITS_TILE, BITS_CAP = 4096, 1024
# the stable append's slot offset of a lane: the passing lanes below it in the ballot bl_
_BALLOT_PREFIX = ("(int)__builtin_amdgcn_mbcnt_hi((unsigned)(bl_ >> 32), "
                  "__builtin_amdgcn_mbcnt_lo((unsigned)bl_, 0u))")


def _scan_args(p: NL.JoinParams, pair: bool = False) -> J.Args:
    """The argument header of both phase-2 generators (the struct layout starts with it);
    ``pair``: with the second query's bitmap and partials (PAIR_SFX)."""
    args = J.Args()
    for n, ct in (("rstart", "const long long*"), ("rlen", "const long long*"),
                  ("tile_prefix", "const long long*")):
        args.add("p", n, ct)
    lk = p.lkey
    args.add("p", f"GM{lk}", "const unsigned long long*")
    args.add("p", f"GR{lk}", "const int*")
    args.add("p", "tags", "const unsigned*")
    if pair:
        args.add("p", "tags" + PAIR_SFX, "const unsigned*")
    args.add("q", "R", "long long")
    args.add("q", "nrows", "long long")
    J._common_args(args)
    if pair:
        for n, ct in (("psum", "double*"), ("pmin", "double*"), ("pmax", "double*"),
                      ("pcnt", "long long*")):
            args.add("p", n + PAIR_SFX, ct)
    return args


# Which bit-parallel phase-2 kernel is generated, resolved once (``_bits_form``): its name; the
# candidate forms' predicate slots ``cand``, whether they keep the passing words (RS_KEEP) and
# serve a pair; a hash / top-K walk; a left-side group table; the predicate slots streamed as
# 12-bit copies; the pipeline depth; ``pack_layout`` of the tail word or None; and the constants:
# T rows per tile, CAP, EW list entries per lane per walk pass (loads in flight together), CC
# candidates per filter pass, KB ring entries and WV wavefronts per workgroup.
# RS_KEEP: a passing candidate's tail word stays in a per-wavefront ring kw_ of KB entries -
# the leftover of a 64-entry group (at most 63) plus one filter pass's appends (at most CC)
_BitsForm = collections.namedtuple(
    "_BitsForm", "name cand keep pair hash topk grouped p12 pipe layout T CAP EW CC KB WV")


def _bits_tail(p: NL.JoinParams, hk, tk) -> list:
    """The slots the walk reads per passing row."""
    # top-K mode segments the walk by key run (lrn_) and loads the key columns only where a
    # group is emitted (jit_hash._hash_accumulate ``seg``): they are not part of the per-row tail
    aggs = J.aggs_of(p)
    return list(dict.fromkeys(J._agg_slots(aggs) + ([p.group_col] if _scan_grouped(p) else []) +
                              (list(hk.slots) if hk is not None and tk is None else [])))


def _bits_form(p: NL.JoinParams, compacts, hk, tk, cand: tuple, pair: bool) -> _BitsForm:
    """The form of ``gen_run_sparse_scan``'s arguments under the bound tunables, and every check
    that the combination exists."""
    grouped = _scan_grouped(p)
    layout = pack_layout(p, compacts, cand)
    keep = bool(cand) and bool(RS_KEEP)
    p12 = () if cand else _p12_slots(p, compacts)
    assert not cand or (hk is None and tk is None)
    assert not pair or cand_pair(p, compacts, cand, hk, tk)
    assert not (grouped and (p.group_col >= SPLIT or hk is not None))
    assert tk is None or hk is not None
    # (the predicates' packed forms, on scratch arguments: the emitters add the literal slots)
    dry = J._Gen(J.Args(), J._col_specs(p, compacts), SPLIT, ("row0", "row0"), frozenset(), True)
    assert not p12 or dry.cnf_sign2(_lpreds(p), "pw{}_", offset="a.P12O_{}") is not None
    if cand:
        assert layout is not None and dry.cnf_sign(_lpreds(p)) is not None
        assert {sl for sl, off, nb in layout if sl in cand and nb == 2} == set(cand)
        # (RS_KEEP: the walk has no row, only the word - every tail slot is one of its fields)
        assert not keep or (not grouped and
                            {sl for sl, _, _ in layout} >= set(_bits_tail(p, hk, tk)))
    name = "hs_jit_run_bits_cand2" if pair else "hs_jit_run_bits_cand" if cand else \
        "hs_jit_run_bits_scan" if hk is None else \
        ("hs_jit_run_bits_hash" if tk is None else "hs_jit_run_bits_topk")
    cc = 64 * max(1, RS_WALK)
    return _BitsForm(name, tuple(cand), keep, bool(pair), hk is not None, tk is not None, grouped,
                     p12, 0 if cand else RS_PIPE, layout, BITS_TILE, BITS_CAP, max(1, RS_WALK),
                     cc, 63 + cc, J.BLOCK // 64)


class _BitsScan:
    """The builder behind ``gen_run_sparse_scan``: one method per stage of the kernel, each
    returning its source lines, over the form ``f``, the argument struct and the column /
    predicate / aggregate descriptions.  Stages add slots to ``args`` as they emit (each says
    so), and the slot order is the ``Args`` struct layout - part of the source text - so the
    order of the driver's calls is fixed: header, ``acc_decls``, ``loads``, ``pred_mask`` or
    ``candidates``, the first ``walk``, ``set_b`` twins where first referenced, ``epilogue``."""

    def __init__(self, p: NL.JoinParams, compacts, hk, tk, cand: tuple, pair: bool):
        self.f = f = _bits_form(p, compacts, hk, tk, cand, pair)
        self.p, self.hk, self.tk, self.lk = p, hk, tk, p.lkey
        self.args = args = _scan_args(p, f.pair)
        self.cols = cols = J._col_specs(p, compacts)
        self.lpreds, self.aggs = _lpreds(p), J.aggs_of(p)
        self.pslots, self.tail = J._pred_slots(self.lpreds), _bits_tail(p, hk, tk)
        self.approx = J._sum_only_slots(self.lpreds, self.aggs,
                                        p.group_col if f.grouped else -1, cols) - \
            set(hk.slots if hk is not None else [])
        self.g1 = J._Gen(args, cols, SPLIT, ("row0", "row0"), self.approx, True)
        self.carry_gen = J._Gen(args, cols, SPLIT, ("tcw_", "tcw_"), frozenset(), True) \
            if tk is not None else None
        self.packed = {sl: (off, nb) for sl, off, nb in f.layout} if f.layout else {}
        # per-query name infix of the tag words, row masks and counts ("" alone: the single forms)
        self.QS = ("", "b") if f.pair else ("",)
        self.elem = {}   # array name -> C expression of element (idx) from its packed 32-bit words
        self.issue = []  # the current tile's (C) tag-word and predicate-column loads into buffer @S@
        self.xpose = []  # RS_LDS: the loaded columns' chunks moved to their rows' lanes
        self.slab = 0    # RS_LDS: 16-byte LDS slots per wavefront

    @staticmethod
    def subst(lines: List[str], ind: str = "", **marks) -> List[str]:
        """``lines`` indented by ``ind`` with the emitters' placeholders replaced, in the order
        given: @S@, the register buffer (A / B) of the tile worked on; @O@, the other buffer,
        which the next tile's loads fill; @T@, the tile index expression; @LIVE@, a prefix of a
        buffer load's byte count ("!nx_ ? 0ll : " empties it past the wavefront's last tile)."""
        out = []
        for x in lines:
            for k, v in marks.items():
                x = x.replace(f"@{k}@", v)
            out.append(ind + x)
        return out

    def set_b(self, lines: List[str]) -> List[str]:
        """``lines`` for the pair's second query: literal slots (twins added as in
        ``gen_run_tags2``), partial pointers and accumulator registers get ``PAIR_SFX``.  The
        regex twin of the first query's code; as a side effect it adds a ``_b`` slot for every
        literal slot it meets first, so the order of its calls fixes the struct layout too."""
        def twin(m):
            kind, name, ct = self.args.slots[self.args._index[m.group(1)]]
            return self.args.add(kind, name + PAIR_SFX, ct)
        return [_ACC_REG.sub(r"\1\2" + PAIR_SFX,
                             _PART_SLOT.sub(r"a.\1" + PAIR_SFX, _LIT_SLOT2.sub(twin, x)))
                for x in lines]

    def at(self, s: str) -> str:
        """Offset of query ``s``'s list in ``lst_`` / ring in ``kw_`` (B's in the union path)."""
        return f"{self.f.KB if self.f.keep else self.f.CAP} + " if s == "b" else ""

    def acc_decls(self) -> List[str]:
        """Accumulators and top-K registers.  Adds num_groups / group_base for a group table."""
        b = J._acc_decls(self.aggs, self.f.grouped, self.args)
        if self.f.pair:
            b += self.set_b(J._acc_decls(self.aggs, self.f.grouped, self.args)[1:])
        if self.tk is not None:
            b += JH._topk_decls(self.aggs, self.tk)
        return b

    def loads(self) -> List[str]:
        """Enumerates the tile's loads - tag words and the predicate columns' row stream (none
        in the candidate forms) - into ``issue`` / ``xpose`` / ``slab`` / ``elem``; returns their
        register buffers' declarations.  Adds the P12_ / P12O_ slots or the column pointers."""
        f, args, b = self.f, self.args, []
        self.issue.append("    { const i64 w_ = (i64)grC >> 5; tw0@S@_ = a.tags[w_]; "
                          "tw1@S@_ = a.tags[w_ + 1]; tw2@S@_ = a.tags[w_ + 2]; }")
        if f.pair:
            self.issue.append("    { const i64 w_ = (i64)grC >> 5; tw0@S@b_ = a.tags_b[w_]; "
                              "tw1@S@b_ = a.tags_b[w_ + 1]; tw2@S@b_ = a.tags_b[w_ + 2]; }")
        for sl in f.p12:
            # 24 dwords (96 bytes) per lane: its 64-row group's 12-bit packed codes
            pp = args.add("p", f"P12_{sl}", "const unsigned*")
            args.add("q", f"P12O_{sl}", "long long")
            b.append(f"  unsigned x{sl}qA[24], x{sl}qB[24];")
            self.issue.append(
                f"    bload<24>(hs_rsrc((const char*){pp} + (tbC >> 6) * 96, "
                f"@LIVE@((a.nrows + 63 - tbC) >> 6) * 96), (unsigned)(ln * 96), x{sl}q@S@);")
        for name, ct, ptr, *_ in ([] if f.p12 or f.cand else J._vec_loads(self.g1, self.pslots)):
            es = J._SIZEOF[ct]
            nw = 64 * es // 4
            per = 4 // es
            b.append(f"  unsigned {name}wA[{nw}], {name}wB[{nw}];")
            # the group's rows past the table end read as 0 (buffer range check); they are outside
            # every row range, so the range mask drops them
            if RS_LDS:
                self.issue.append(f"    bload_t<{nw}>(hs_rsrc((const char*){ptr} + tbC * {es}, "
                                  f"@LIVE@(a.nrows - tbC) * {es}), ln, {name}w@S@);")
                self.xpose.append(f"    hs_lds_t<{nw}>(&xt_[wq][0], ln, {name}w@S@);")
                self.slab = max(self.slab, nw // 4 * 64)
            else:
                self.issue.append(f"    bload<{nw}>(hs_rsrc((const char*){ptr} + tbC * {es}, "
                                  f"@LIVE@(a.nrows - tbC) * {es}), (unsigned)(64 * ln * {es}), "
                                  f"{name}w@S@);")
            self.elem[name] = (ct, f"{name}w@S@[({{i}}) / {per}]" if per > 1
                               else f"{name}w@S@[{{i}}]", 8 * es, per)
        return b

    def lds_decls(self) -> List[str]:
        """The LDS arrays and the nibble table's fill; after ``loads``, which sizes RS_LDS's slab."""
        f, b = self.f, []
        WV, CAP, CC, KB = f.WV, f.CAP, f.CC, f.KB  # noqa: N806
        if f.topk:
            b.append(f"  __shared__ unsigned short lrn_[{WV}][{CAP}];")
        if RS_LUT:
            # dlut_[m | w << 4]: the 4 row tags of a nibble with run-start bits m, tag window w
            b += ["  __shared__ unsigned char dlut_[512];",
                  f"  for (int e_ = (int)threadIdx.x; e_ < 512; e_ += {J.BLOCK}) {{",
                  "    unsigned k_ = 0u, o_ = 0u;",
                  "    for (int j_ = 0; j_ < 4; ++j_) { k_ += (e_ >> j_) & 1; "
                  "o_ |= (((unsigned)e_ >> (4u + k_)) & 1u) << j_; }",
                  "    dlut_[e_] = (unsigned char)o_; }",
                  "  __syncthreads();"]
        if f.cand:
            b.append(f"  __shared__ unsigned short clst_[{WV}][{CC}];")
        if f.keep:
            # (pair form: A's ring at 0 and B's at KB; the dense path uses A's for one query at a time)
            b.append(f"  __shared__ u64 kw_[{WV}][{(2 if f.pair else 1) * KB}];")
        elif self.xpose:
            # the transpose slab and the passing-row list share the LDS: a tile's list is built
            # after its columns left the slab, and walked before the next tile's transpose
            nslot = max(self.slab, (CAP * 2 + 15) // 16)
            # lst_[w] = wavefront w's own slab, seen as 16-bit entries
            b += [f"  __shared__ hs_v4u xt_[{WV}][{nslot}];",
                  f"  unsigned short (*lst_)[{nslot * 8}] = "
                  f"(unsigned short (*)[{nslot * 8}])&xt_[0][0];"]
        else:
            # (pair form: A's list at 0 and B's at CAP in the union path; the dense path uses
            # [0, CAP + CC) for one query at a time)
            b.append(f"  __shared__ unsigned short lst_[{WV}]"
                     f"[{((2 if f.pair else 1) * CAP + CC) if f.cand else CAP}];")
        return b

    def split(self) -> List[str]:
        """The wavefront's tiles, its first tile's row range (binary search), pipeline registers."""
        WV = self.f.WV  # noqa: N806
        return ["  const int ln = (int)(threadIdx.x & 63);",
                "  const int wq = (int)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));",
                "  const i64 ntiles = a.tile_prefix[a.R];",
                f"  const i64 nwv = (i64)gridDim.x * {WV};",
                f"  const i64 wid = (i64)blockIdx.x * {WV} + wq;",
                "  const i64 per = (ntiles + nwv - 1) / nwv;",
                "  const i64 t0 = wid * per;",
                "  const i64 t1 = ntiles < t0 + per ? ntiles : t0 + per;",
                "  int r = 0;",
                "  if (t0 < t1) { int lo = 0, hi = (int)a.R;",
                "    while (hi - lo > 1) { const int m = (lo + hi) >> 1; "
                "if (a.tile_prefix[m] <= t0) lo = m; else hi = m; }",
                "    r = lo; }",
                # software pipeline (RS_PIPE), one exposed memory round trip per tile: tile t's tag
                # words and predicate columns were issued during tile t-1 (after its masks were
                # formed, before its list walk, so the walk's aggregate-input loads wait on them
                # together) and the run-form words of tile t+1 one tile earlier still (the tag words'
                # address needs them).  The tile loop is unrolled by two over two named buffers (A, B):
                # a loop-carried array is copied register to register at the back edge otherwise,
                # after a wait for its loads, and held twice.
                "  i64 rsC = 0, reC = 0, tbC = 0; u64 gmC = 0ull; int grC = 0;",
                "  i64 rsN = 0, reN = 0, tbN = 0; u64 gmN = 0ull; int grN = 0;",
                "  unsigned tw0A_ = 0u, tw1A_ = 0u, tw2A_ = 0u, tw0B_ = 0u, tw1B_ = 0u, tw2B_ = 0u;"] + \
            (["  unsigned tw0Ab_ = 0u, tw1Ab_ = 0u, tw2Ab_ = 0u;"] if self.f.pair else [])

    def geom(self, tv: str, sfx: str) -> List[str]:
        """Tile ``tv``'s range / row geometry and its group's run-form words (suffix sfx).  The
        words stay in their loaded types (no OR / widening here): an operation on a loaded value
        makes the compiler wait for the load on the spot, and these are prefetched a tile ahead."""
        lk = self.lk
        return [f"    while (r + 1 < (int)a.R && a.tile_prefix[r + 1] <= {tv}) ++r;",
                f"    rs{sfx} = a.rstart[r]; re{sfx} = rs{sfx} + a.rlen[r];",
                f"    tb{sfx} = (rs{sfx} & ~(i64)63) + ({tv} - a.tile_prefix[r]) * {self.f.T};",
                f"    {{ const i64 r0_ = tb{sfx} + 64 * ln; "
                f"const i64 g_ = (r0_ < a.nrows ? r0_ : a.nrows - 1) >> 6;",
                f"      gm{sfx} = a.GM{lk}[g_]; gr{sfx} = a.GR{lk}[g_]; }}"]

    def prologue(self) -> List[str]:
        """The first tile's geometry (pipelined: its loads and the second tile's geometry too).
        The next tile's run-form words are prefetched during the current tile."""
        b = ["  if (t0 < t1) {"]
        if self.f.pipe:
            b += self.geom("t0", "C")
            b += self.subst(self.issue, S="A", LIVE="")
            b += ["    if (t0 + 1 < t1) {"]
            b += self.subst(self.geom("(t0 + 1)", "N"), "  ")
            b += ["    }"]
        else:
            b += self.geom("t0", "N")
        return b + ["  }"]

    def tile_rows(self) -> List[str]:
        """Head of a tile's body: (not pipelined) its loads, then the lane's 64 rows, the part
        ``am`` of them inside the tile's row range, and the tag window's shift."""
        body: List[str] = []
        if not self.f.pipe:
            # this tile's loads, then the next tile's run-form words: two round trips per tile (the
            # column stream, then the walk's aggregate inputs), fewer registers
            body += ["    rsC = rsN; reC = reN; tbC = tbN; gmC = gmN; grC = grN;"]
            body += self.subst(self.issue, LIVE="")
            body += ["    if (@T@ + 1 < t1) {"]
            body += self.subst(self.geom("(@T@ + 1)", "N"), "  ")
            body += ["    }"]
        body += ["    const i64 rs = rsC, re = reC, tb0 = tbC; const u64 m_ = gmC | 1ull; "
                 "const i64 q0 = (i64)grC;"]
        if self.f.topk:
            # key run of a list entry, relative to the tile's first run (lrn_)
            body.append("    const i64 qb_ = __shfl(q0, 0, 64); const int qr_ = (int)(q0 - qb_);")
        body += ["    const i64 row0 = tb0 + 64 * ln;",
                 "    const i64 lo_ = rs - row0, hi_ = re - row0;",
                 "    const int alo = lo_ <= 0 ? 0 : (lo_ >= 64 ? 64 : (int)lo_);",
                 "    const int ahi = hi_ <= 0 ? 0 : (hi_ >= 64 ? 64 : (int)hi_);",
                 "    const u64 am = alo >= ahi ? 0ull : ((ahi == 64 ? ~0ull : ((1ull << ahi) - 1ull)) & "
                 "~((1ull << alo) - 1ull));",
                 "    const unsigned sh_ = (unsigned)(q0 & 31);"]
        return body

    def tag_mask(self) -> List[str]:
        """Step 1, the tag mask d<q>_: the tag bits of the group's runs (gruns / 3 tag words)
        deposited at the run starts (gmask) and spread over each run's rows, limited to the
        tile's range rows - ~1.5 instructions per row."""
        body = []
        for q in self.QS:
            body += [f"    const u64 lw{q}_ = (u64)tw0@S@{q}_ | ((u64)tw1@S@{q}_ << 32);",
                     f"    const u64 hw{q}_ = (u64)tw2@S@{q}_;",
                     f"    const u64 T{q}_ = sh_ ? ((lw{q}_ >> sh_) | (hw{q}_ << (64 - sh_))) : lw{q}_;"]
        return body + (self.tag_mask_lut() if RS_LUT else self.tag_mask_loop())

    def tag_mask_lut(self) -> List[str]:
        # row tags by nibble: rows 4i..4i+3 take their tags from a 5-run window of T (the run
        # covering row 4i-1, then the runs starting in the nibble) through a 512-entry LDS
        # table indexed by (nibble of run starts, window) - 16 fixed steps instead of a loop
        # over the group's run starts (~15 VALU per start, ~20-28 starts for the slowest lane)
        # (pair form: the run starts and their running count are shared, one lookup per query)
        QS = self.QS  # noqa: N806
        body = [f"    u64 d{q}_ = (u64)dlut_[((unsigned)m_ & 15u) | "
                f"((((unsigned)T{q}_ << 1) & 31u) << 4)];" for q in QS]
        body += ["    unsigned P_ = (unsigned)__popc((unsigned)m_ & 15u);",
                 "    #pragma unroll",
                 "    for (int i_ = 1; i_ < 16; ++i_) {",
                 "      const unsigned mn_ = (unsigned)(m_ >> (4 * i_)) & 15u;"]
        for q in QS:
            body += [f"      const unsigned ix{q}_ = mn_ | "
                     f"(((unsigned)(T{q}_ >> (P_ - 1u)) & 31u) << 4);",
                     f"      d{q}_ |= (u64)dlut_[ix{q}_] << (4 * i_);"]
        body += ["      P_ += (unsigned)__popc(mn_);",
                 "    }"]
        return body + [f"    d{q}_ &= am;" for q in QS]

    def tag_mask_loop(self) -> List[str]:
        """The loop form: one step per run start of the group, then a prefix XOR spreads each
        run's tag over its rows (as hs_run_rowmask)."""
        return [
             # only the group's own runs' tags (popc(m) of them) decide whether any row is set
             "    const int nr_ = __popcll(m_);",
             "    const u64 Tm_ = nr_ >= 64 ? T_ : (T_ & ((1ull << nr_) - 1ull));",
             "    u64 c_ = T_ ^ (T_ << 1), d_ = 0ull, mm_ = (am && Tm_) ? m_ : 0ull;",
             "    while (mm_) { const u64 lb_ = mm_ & (0ull - mm_); if (c_ & 1ull) d_ |= lb_; "
             "c_ >>= 1; mm_ ^= lb_; }",
             "    d_ ^= d_ << 1; d_ ^= d_ << 2; d_ ^= d_ << 4; d_ ^= d_ << 8; d_ ^= d_ << 16; "
             "d_ ^= d_ << 32;",
             "    d_ &= am;"]

    def pred_mask(self) -> List[str]:
        """Step 2, the predicate mask: the lane's 64 rows of every left predicate column (vector
        loads, in flight with the tag words), one compare + shift-or per row, ANDed into d_.
        Adds the predicates' literal slots (``cnf`` first, then the sign forms')."""
        g1, lpreds, pslots = self.g1, self.lpreds, self.pslots
        # predicate mask: 64 compares, shift-or into two 32-bit halves (a C loop: each row's
        # value is decoded where it is compared, not all 64 held decoded at once)
        body = ["    unsigned plo_ = 0u, phi_ = 0u;"]
        cond = J._rename(g1.cnf(lpreds), pslots, "k")
        # narrow compact-code ranges: fail bits from a sign word (no compares, no constants held in
        # registers for the select), else the generic condition's pass bits
        sign = g1.cnf_sign(lpreds)
        if sign is not None:
            sign = J._rename(sign, pslots, "k")
        # two rows per 32-bit word (16-bit signed codes): packed saturating range tests, fail bits
        # gathered in even/odd order per 32-row half, then unzipped (2.5 VALU per row instead of 5)
        sign2 = g1.cnf_sign2(lpreds, "x{}w@S@[w_]") if RS_PK16 and sign is not None and \
            all(J._SIZEOF.get(g1.raw_type(sl)) == 2 for sl in pslots) else None
        if self.f.p12:
            body += self.pred_mask_p12()
        elif sign2 is not None:
            body += self.pred_mask_pk16(sign2)
        else:
            body += self.pred_mask_rows(cond, sign)
        if sign is not None:
            body += ["    d_ &= ~(((u64)phi_ << 32) | (u64)plo_);"]
        else:
            body += ["    d_ &= ((u64)phi_ << 32) | (u64)plo_;"]
        return body

    def pred_mask_p12(self) -> List[str]:
        # 12-bit chunks: decode 8 rows per 3 dwords, pair them into 16-bit halves, packed tests
        p12 = self.f.p12
        sign12 = self.g1.cnf_sign2(self.lpreds, "pw{}_", offset="a.P12O_{}")
        body = []
        for i in range(8):
            body.append("    {")
            for sl in p12:
                body += [f"      const unsigned a{sl}_ = x{sl}q@S@[{3 * i}], "
                         f"b{sl}_ = x{sl}q@S@[{3 * i + 1}], c{sl}_ = x{sl}q@S@[{3 * i + 2}];",
                         f"      const unsigned v{sl}_0 = a{sl}_ & 0xFFFu, "
                         f"v{sl}_1 = (a{sl}_ >> 12) & 0xFFFu, "
                         f"v{sl}_2 = ((a{sl}_ >> 24) | (b{sl}_ << 8)) & 0xFFFu, "
                         f"v{sl}_3 = (b{sl}_ >> 4) & 0xFFFu;",
                         f"      const unsigned v{sl}_4 = (b{sl}_ >> 16) & 0xFFFu, "
                         f"v{sl}_5 = ((b{sl}_ >> 28) | (c{sl}_ << 4)) & 0xFFFu, "
                         f"v{sl}_6 = (c{sl}_ >> 8) & 0xFFFu, v{sl}_7 = c{sl}_ >> 20;"]
            for q in range(4):
                w = 4 * i + q
                half, wl = ("plo_", w) if w < 16 else ("phi_", w - 16)
                body.append("      {")
                for sl in p12:
                    body.append(f"        const unsigned pw{sl}_ = v{sl}_{2 * q} | "
                                f"(v{sl}_{2 * q + 1} << 16);")
                body += [f"        const unsigned s2_ = {sign12};",
                         f"        {half} |= (s2_ >> {15 - wl}) & {(1 << wl) | (1 << (wl + 16))}u;",
                         "      }"]
            body.append("    }")
        return body + ["    plo_ = hs_unzip16(plo_);", "    phi_ = hs_unzip16(phi_);"]

    def pred_mask_pk16(self, sign2: str) -> List[str]:
        """16-bit codes, two rows per loaded word (``sign2``: their packed range test)."""
        body = []
        for half, off in (("plo_", 0), ("phi_", 16)):
            body += ["    #pragma unroll",
                     "    for (int w_ = 0; w_ < 16; ++w_) {",
                     f"      const unsigned s2_ = {sign2.replace('[w_]', f'[w_ + {off}]')};",
                     f"      {half} |= (s2_ >> (15 - w_)) & ((1u << w_) | (1u << (w_ + 16)));",
                     "    }",
                     f"    {half} = hs_unzip16({half});"]
        return body

    def pred_mask_rows(self, cond: str, sign: Optional[str]) -> List[str]:
        """Any predicate, row by row: each column's element from its packed words, decoded, then
        the sign test's fail bit or ``cond``'s pass bit.  Adds B<slot> of a based compact code."""
        g1, cols, body = self.g1, self.cols, []

        def raw_of(name: str, off: int) -> str:
            et, word, bits, per = self.elem[name]
            i = f"{off} + k_"
            w = word.format(i=i)
            return f"(({et})({w} >> ({bits} * (({i}) % {per}))))" if per > 1 else f"(({et}){w})"
        for half, off in (("plo_", 0), ("phi_", 32)):
            body.append("    #pragma unroll")
            body.append("    for (int k_ = 0; k_ < 32; ++k_) {")
            for sl in self.pslots:
                ct = J._CTYPE[cols[sl][0]]
                enc = cols[sl][2]
                raw = raw_of(f"x{sl}", off)
                body.append(f"      const auto xr{sl}_k = {raw};")
                raw = f"xr{sl}_k"
                if enc:
                    body.append(f"      const int r{sl}_k = (int){raw};")
                if enc and enc[1]:
                    bq = self.args.add("q", f"B{sl}", "long long")
                    body.append(f"      const i64 q{sl}_k = {bq} + (i64){raw};")
                body.append(f"      const {ct} x{sl}_k = {g1.decode(sl, raw)};")
                if cols[sl][1]:
                    body.append(f"      const bool n{sl}_k = {raw_of(f'n{sl}', off)} != 0;")
            if sign is not None:
                body.append(f"      {half} |= ((unsigned)({sign}) >> 31) << k_;")
            else:
                body.append(f"      {half} |= ({cond} ? 1u : 0u) << k_;")
            body.append("    }")
        return body

    def prefetch(self) -> List[str]:
        """RS_PIPE: the next tile's loads into the other buffer, and the geometry of the tile
        after it."""
        # this tile's column words are consumed: the next tile's loads go out now
        # (the scheduler must not hoist the next tile's loads above this tile's masks: both
        # buffers would be live at once)
        # The loads are unconditional - a load under a condition keeps the buffer's previous
        # contents live through the whole tile - and past the wavefront's last tile they read
        # an empty buffer range (no memory traffic; the tag words re-read this tile's).
        return ["    __builtin_amdgcn_sched_barrier(0);",
                "    { const bool nx_ = @T@ + 1 < t1;",
                "      if (nx_) { rsC = rsN; reC = reN; tbC = tbN; gmC = gmN; grC = grN; }"] + \
            self.subst(self.issue, "  ", S="@O@", LIVE="!nx_ ? 0ll : ") + \
            ["      if (@T@ + 2 < t1) {"] + \
            self.subst(self.geom("(@T@ + 2)", "N"), "    ") + \
            ["      }", "    }"]

    def scan(self, q: str, tot: bool = True) -> List[str]:
        """Exclusive scan of the lanes' counts of row mask d<q>_ (cn / inc / tot <q>_)."""
        return [f"    const int cn{q}_ = __popcll(d{q}_);",
                f"    int inc{q}_ = cn{q}_;",
                f"    for (int o_ = 1; o_ < 64; o_ <<= 1) {{ const int y_ = __shfl_up(inc{q}_, o_, 64); "
                f"if (ln >= o_) inc{q}_ += y_; }}"] + \
            ([f"    const int tot{q}_ = __shfl(inc{q}_, 63, 64);"] if tot else [])

    def walk(self, at: str = "", hp: str = "hp_") -> List[str]:
        """Step 3's second half.  The walk of list entries [0, wn_) of ``lst_`` (from element
        ``at`` on): entry cb + 64 k + ln goes to lane ln, k ascending; aggregate inputs loaded at
        those rows only and accumulated.  RS_KEEP: of the wn_ ring entries of ``kw_`` (ring at
        ``at``) from slot ``hp`` on; the entries are the tail words themselves.

        With ``hk`` (an exec.hash_agg.KeyPlan over left columns) the walk groups by the hash key
        instead: each pass's 64 list entries are consecutive passing rows, so a segmented shuffle
        reduce folds a group's rows (one run = one left join key) before one table probe
        (``jit_hash._hash_accumulate``); kernel ``hs_jit_run_bits_hash``, no partials.

        With ``tk`` as well (an exec.hash_agg.TopKPlan: ORDER BY <aggregate> LIMIT k over those
        groups), the windows are walked in row order with the last segment of each carried into
        the next (``jit_hash._topk_accumulate``): a key is final when the walk leaves it and
        competes for the wavefront's top-K registers instead of probing the table; only keys that
        may continue into the neighbouring wavefronts' tiles (at most two per wavefront) go to
        the table (kernel ``hs_jit_run_bits_topk``; every wavefront writes its list at the end).

        Adds (first call) PK, group_base, num_groups, B<slot> and what the accumulation adds."""
        f, p, args, tail, tk = self.f, self.p, self.args, self.tail, self.tk
        keep, layout, packed, KB = f.keep, f.layout, self.packed, f.KB  # noqa: N806
        # (RS_KEEP: LDS reads need no batch in flight - one entry per lane and step, fewer registers)
        WE = 1 if keep else f.EW  # noqa: N806
        w = [f"    for (int cb = 0; cb < wn_; cb += {64 * WE}) {{"]
        if layout and not keep:
            w.append("      const u64* PKt_ = a.PK + tb0;")
        ind2 = "      "
        for k in range(WE):
            w += [f"{ind2}const int ce{k} = cb + {64 * k} + ln;",
                  f"{ind2}const bool cok{k} = ce{k} < wn_;"]
            if keep:
                # (hp < KB and ce < wn_ <= KB: one conditional subtraction wraps)
                w += [f"{ind2}const int ci{k} = {hp} + ce{k} - ({hp} + ce{k} >= {KB} ? {KB} : 0);",
                      f"{ind2}const u64 pk{k}_ = cok{k} ? kw_[wq][{at}ci{k}] : 0ull;"]
                continue
            w += [f"{ind2}const int cof{k} = cok{k} ? (int)lst_[wq][{at}ce{k}] : 0;",
                  f"{ind2}const i64 crow{k} = tb0 + (i64)cof{k};"]
            if tk is not None:
                w.append(f"{ind2}const unsigned crn{k} = cok{k} ? (unsigned)lrn_[wq][ce{k}] : "
                         f"0xFFFFFFFFu;")
        gs = [J._Gen(args, self.cols, SPLIT, (f"crow{k}", f"crow{k}"), self.approx, True)
              for k in range(WE)]
        if layout:
            args.add("p", "PK", "const unsigned long long*")
        for k in range(WE):
            if layout and not keep:
                # the tile's rows through a uniform base: 32-bit lane offsets
                w.append(f"{ind2}const u64 pk{k}_ = PKt_[cof{k}];")
            for sl in tail:
                if sl in packed:
                    off, nb = packed[sl]
                    ct = gs[k].raw_type(sl)
                    ut = {1: "unsigned char", 2: "unsigned short", 4: "unsigned"}[nb]
                    J._uload_raw(gs[k], sl, f"c{k}", f"(({ct})({ut})(pk{k}_ >> {off}))", "1", w,
                                 ind2)
                else:
                    J._uload(gs[k], sl, f"c{k}", w, ind2)
        for k in range(WE):
            g = gs[k]
            it = f"c{k}"
            w.append(f"{ind2}{{ bool cok = cok{k};")
            gvar = "gic"
            if f.grouped:
                w += g.group_index(p.group_col, it, "cok", ind2, ("glc", gvar))
            if self.hk is not None:
                w += [J._rename(x, tail, it)
                      for x in JH._hash_accumulate(g, self.aggs, self.hk, "cok", ind2, tk=tk,
                                                   seg=f"crn{k}" if tk is not None else None,
                                                   row=f"crow{k}", run=f"qb_ + (i64)crn{k}",
                                                   carry_gen=self.carry_gen)]
            else:
                w += [J._rename(x, tail, it)
                      for x in J._accumulate(g, self.aggs, f.grouped, "cok", gvar, ind2)]
            w.append(f"{ind2}}}")
        w.append("    }")
        return w

    def stream_fill(self) -> List[str]:
        """Step 3's first half, the streaming forms: the rows of (tag mask & predicate mask) -
        the join's passing rows, a few percent - go to a per-wavefront LDS list (offsets from a
        shuffle scan of the lanes' popcounts), which the wavefront walks EW entries per lane per
        pass, CAP entries a round."""
        CAP = self.f.CAP  # noqa: N806
        return [
          f"    for (int wb_ = 0; wb_ < tot_; wb_ += {CAP}) {{",
          f"    const int wn_ = tot_ - wb_ < {CAP} ? tot_ - wb_ : {CAP};",
          "    { int pos_ = inc_ - cn_ - wb_; u64 e_ = d_;",
          "      while (e_) { const int bq_ = __builtin_ctzll(e_); "
          f"if (pos_ >= 0 && pos_ < {CAP}) {{ lst_[wq][pos_] = (unsigned short)(64 * ln + bq_); "
          + ("lrn_[wq][pos_] = (unsigned short)(qr_ + __popcll(m_ & ((2ull << bq_) - 1ull))); "
             if self.f.topk else "") +
          "} ++pos_; e_ &= e_ - 1ull; } }",
          f"    {J._wave_sync(False)}"] + self.walk() + [f"    {J._wave_sync(False)}", "    }"]

    def append(self, k: int, ok: str, s: str) -> List[str]:
        """Stable append (ballot + prefix count) of pass entry k's row for query ``s`` ("" the
        single forms' / the dense path's, "a" / "b" the union path's) if it is a candidate of
        the query (``ok``) and passes the left predicates.  Listing form: its row offset goes to
        ``lst_`` at np<s>_ + prefix.  RS_KEEP: its tail word to ring slot (np + prefix) % KB.
        Per query four wavefront-uniform counters: np entries appended since the last
        reset (what ``np_ <= CAP`` tests, as in the listing form), ch of them consumed - a
        multiple of 64, so entry e still goes to lane e % 64 - and kp / hp, the ring slots of
        entries np / ch (np, ch modulo KB, kept by conditional subtraction)."""
        KB, at = self.f.KB, self.at(s)  # noqa: N806
        out = [f"      {{ const bool fp_ = {ok} && "
               f"(int)({J._rename(self.sign, self.pslots, f'f{k}')}) >= 0;",
               "        const u64 bl_ = __ballot(fp_);"]
        if not self.f.keep:
            return out + [
                f"        if (fp_) lst_[wq][{at}np{s}_ + {_BALLOT_PREFIX}] = (unsigned short)fof{k};",
                f"        np{s}_ += __popcll(bl_); }}"]
        return out + [
            f"        const int ix_ = kp{s}_ + {_BALLOT_PREFIX};",
            f"        if (fp_) kw_[wq][{at}ix_ - (ix_ >= {KB} ? {KB} : 0)] = fw{k}_;",
            f"        const int nb_ = __popcll(bl_); np{s}_ += nb_; kp{s}_ += nb_; "
            f"if (kp{s}_ >= {KB}) kp{s}_ -= {KB}; }}"]

    def filter_pass(self, q: str, entry: str, appends, member: bool = False) -> List[str]:
        """One filter pass of the candidate forms: candidates [wb_, wb_ + CC) of row mask d<q>_
        (in row order) -> ``clst_`` as ``entry`` (of lane ln's row bq_), each candidate's
        row-packed tail word loaded (it holds the predicate columns' codes as extra fields), the
        fields taken out, and ``appends(k)``: the stable append(s) of pass entry k.  ``member``:
        the entry carries membership bits (fen<k>) over its 12-bit row offset (the union path)."""
        f, sync = self.f, J._wave_sync(True)
        CC, EW = f.CC, f.EW  # noqa: N806
        fields = {sl: off for sl, off, nb in f.layout if sl in f.cand and nb == 2}
        c = [f"      {{ int pos_ = inc{q}_ - cn{q}_ - wb_; u64 e_ = (pos_ < " + str(CC) +
             f" && pos_ + cn{q}_ > 0) ? d{q}_ : 0ull;",
             "        while (e_) { const int bq_ = __builtin_ctzll(e_); "
             f"if (pos_ >= 0 && pos_ < {CC}) clst_[wq][pos_] = (unsigned short)({entry}); "
             "++pos_; e_ &= e_ - 1ull; } }",
             f"      {sync}",
             f"      const int cw_ = tot{q}_ - wb_ < {CC} ? tot{q}_ - wb_ : {CC};"]
        for k in range(EW):
            c.append(f"      const bool fok{k} = {64 * k} + ln < cw_;")
            if member:
                c += [f"      const int fen{k} = fok{k} ? (int)clst_[wq][{64 * k} + ln] : 0;",
                      f"      const int fof{k} = fen{k} & 4095;"]
            else:
                c.append(f"      const int fof{k} = fok{k} ? (int)clst_[wq][{64 * k} + ln] : 0;")
        for k in range(EW):
            c.append(f"      const u64 fw{k}_ = PKc_[fof{k}];")
        c.append(f"      {sync}")
        for k in range(EW):
            c += [f"      const int r{sl}_f{k} = (int)(short)(unsigned short)(fw{k}_ >> {off});"
                  for sl, off in fields.items()] + appends(k)
        return c

    def consume(self, s: str, fin: str) -> List[str]:
        """RS_KEEP.  Sum the pending entries' whole groups of 64 - all of them where ``fin`` -
        from query ``s``'s ring: the walk of [ch, ch + wn_), in the listing form's order."""
        KB = self.f.KB  # noqa: N806
        w = self.walk(self.at(s), f"hp{s}_")
        return [f"    {{ const int wn_ = ({fin} ? np{s}_ : (np{s}_ & ~63)) - ch{s}_;"] + \
            (self.set_b(w) if s == "b" else w) + \
            [f"      ch{s}_ += wn_; hp{s}_ += wn_; if (hp{s}_ >= {KB}) hp{s}_ -= {KB}; }}"]

    def cand_loop(self, q: str) -> List[str]:
        """One query's candidate loop over the tile (the single form's): filter passes of CC
        candidates; the walk runs once per tile, after its last candidate (so a tile's
        passing-row sequence, and with it every lane's sum order, is that of the streaming form
        while the tile has at most CAP passing rows), or earlier whenever ``lst_`` holds more
        than CAP entries (a pass adds at most CC).  That is the *listing form* (RS_KEEP off): its
        walk loads the tail word of a passing row again (an L2 hit a few hundred cycles after the
        filter's load) - one more dependent round trip per tile.

        With RS_KEEP (the default) the filter pass keeps the word instead: the stable append
        writes the 64-bit word ``fw<k>_`` of a passing entry into a per-wavefront ring ``kw_`` at
        slot (entries appended since the last reset + ballot prefix) mod KB, and nothing into
        ``lst_``, which goes.  The walk hands entry e (counted since the reset) to lane e % 64 in
        ascending order, so any complete group of 64 entries can be summed as soon as it exists:
        after every pass the ``cb`` loop takes the pending whole groups from the ring (its head
        stays a multiple of 64), and the rest where the listing form walks (``fin_``) - after the
        tile's last pass, or once more than CAP entries were appended since the reset (``np_``
        still counts appended, not pending, entries, so resets and with them the lane of every
        later entry fall where they fell).  Each lane therefore adds the same values in the same
        order; a different number of masked-off slots only adds +0.0 to sums that start at +0.0.
        KB = 63 + CC: the most a ring can hold before a consumption (a leftover below 64 plus one
        pass's CC appends) - 2.5 KB per wavefront instead of 8 (CAP + CC) for a whole tile's
        words.  Every tail slot is a field of the word (``pack_layout`` is required here), so the
        walk keeps no row offset and issues no global load; it takes one entry per lane and step
        (LDS reads need no batch in flight), which with the addresses and in-flight loads gone
        brings the single form from 70 to 62 VGPRs."""
        f, sync = self.f, J._wave_sync(True)
        keep, CAP, CC = f.keep, f.CAP, f.CC  # noqa: N806
        more = f"wb_ < tot{q}_ && np_ <= {CAP}"
        c = ["    int np_ = 0, wb_ = 0" + (", kp_ = 0, ch_ = 0, hp_ = 0;" if keep else ";"),
             "    for (;;) {",
             f"    if (wb_ < tot{q}_) {{"]
        c += self.filter_pass(q, "64 * ln + bq_", lambda k: self.append(k, f"fok{k}", ""))
        c += [f"      wb_ += {CC};"] + ([] if keep else [f"      if ({more}) continue;"]) + ["    }"]
        if keep:
            c += [f"    const bool fin_ = !({more});", f"    {sync}"] + self.consume("", "fin_") + \
                [f"    {sync}",
                 "    if (fin_) { np_ = 0; kp_ = 0; ch_ = 0; hp_ = 0; "
                 f"if (wb_ >= tot{q}_) break; }}"]
        else:
            c += ["    const int wn_ = np_;", f"    {sync}"] + self.walk() + \
                [f"    {sync}", "    np_ = 0;", f"    if (wb_ >= tot{q}_) break;"]
        return c + ["    }"]

    def pair_union(self) -> List[str]:
        """Pair form, a tile in which neither query has more than CAP candidates - every tile of
        the headline: the candidates of (mask A | mask B) go through ``clst_`` with two
        membership bits beside the 12-bit row offset, each tail word is loaded once, either
        query's predicates are tested with its literals under its membership bit, and the two
        stable appends fill two lists (A at 0, B at CAP of one ``lst_`` of 2 CAP + CC entries:
        neither can exceed CAP).  After the tile's last pass the single form's walk runs over A's
        list into A's accumulators, then over B's into B's: the single form would not have walked
        earlier either, so every lane adds the same values in the same order.  With RS_KEEP the
        union path has two rings (A's at 0, B's at KB of one ``kw_``) and sums A's whole groups,
        then B's, after every pass."""
        f, sync = self.f, J._wave_sync(True)
        body = ["    const u64 du_ = d_ | db_;"] + self.scan("u")
        body += ["    int npa_ = 0, npb_ = 0;"] + \
            (["    int kpa_ = 0, cha_ = 0, hpa_ = 0, kpb_ = 0, chb_ = 0, hpb_ = 0;"]
             if f.keep else []) + \
            [f"    for (int wb_ = 0; wb_ < totu_; wb_ += {f.CC}) {{"]
        # entry: row offset (12 bits), bit 12: a candidate of A, bit 13: of B
        body += self.filter_pass(
            "u", "(64 * ln + bq_) | (int)((d_ >> bq_) & 1ull) << 12 | "
            "(int)((db_ >> bq_) & 1ull) << 13",
            lambda k: self.append(k, f"(fen{k} & 4096)", "a") +
            self.set_b(self.append(k, f"(fen{k} & 8192)", "b")), member=True)
        if f.keep:
            # whole groups after every pass, the rest after the tile's last: A's, then B's
            return body + [f"      const bool fin_ = wb_ + {f.CC} >= totu_;", f"      {sync}"] + \
                self.consume("a", "fin_") + self.consume("b", "fin_") + [f"      {sync}", "    }"]
        return body + ["    }", f"    {sync}",
                       "    { const int wn_ = npa_;"] + self.walk() + ["    }",
                       "    { const int wn_ = npb_;"] + self.set_b(self.walk(self.at("b"))) + \
            ["    }", f"    {sync}"]

    def candidates(self) -> List[str]:
        """Step 3's first half, the candidate forms (``cand``: the predicate slots of
        ``prune_plan``; kernel ``hs_jit_run_bits_cand``): phase 1 tagged only runs that may hold a
        passing row, so step 2's row stream goes.  The rows of (tag mask & range mask) are the
        tile's *candidates*; they go to a small per-wavefront LDS list ``clst_``, 64 * RS_WALK at
        a time, the wavefront loads each candidate's row-packed tail word, tests the left
        predicates on its fields and appends the passing entries stably to ``lst_`` (or their
        words to the ring), which the walk consumes (``filter_pass``, ``cand_loop``).

        Pair form (``pair``, ``cand_pair``; kernel ``hs_jit_run_bits_cand2``): two queries tagged
        by the pair phase 1 (bitmaps ``tags`` / ``tags_b``, the second literal set and partials
        with ``PAIR_SFX``) in one pass over the same tiles.  Both row masks come from one LUT
        expansion of the shared run starts.  A tile takes the *union path* (``pair_union``) or the
        *dense path*: the single form's candidate loop, emitted by the same code, once per query
        (its early walks depend on where the candidate batches fall, which a union pass cannot
        reproduce; RS_KEEP: it uses A's ring for one query at a time).  Grid, tile split and
        flush are the single form's, so each query's partials are bit for bit those of its own
        launch.  Adds the left predicates' literal slots (``cnf_sign``), before the first walk's."""
        # candidates -> clst_ (CC per pass) -> tail word -> left predicates on its fields ->
        # stable append to lst_; the walk runs after the tile's last pass (or when lst_
        # holds more than CAP entries: a pass adds at most CC)
        CAP = self.f.CAP  # noqa: N806
        self.sign = self.g1.cnf_sign(self.lpreds)
        body = ["    const u64* PKc_ = a.PK + tb0;"]
        if not self.f.pair:
            return body + self.cand_loop("")
        # union path: both queries at most CAP candidates in the tile (wavefront-uniform)
        return body + [f"    if (tot_ <= {CAP} && totb_ <= {CAP}) {{   // union path"] + \
            self.pair_union() + ["    } else {   // dense path", "    {"] + \
            self.scan("", False) + self.cand_loop("") + ["    }", "    {"] + \
            self.scan("b", False) + self.set_b(self.cand_loop("b")) + ["    }", "    }"]

    def tile_body(self) -> List[str]:
        """One tile (@T@), its buffer @S@, the next tile's buffer @O@ (``subst``)."""
        f = self.f
        body = self.tile_rows() + self.tag_mask() + self.xpose
        # (the candidate form tests the predicates per candidate row, on its tail word)
        if not f.cand:
            body += self.pred_mask()
        if f.pipe:
            body += self.prefetch()
        if not f.pair:
            return body + self.scan("") + (self.candidates() if f.cand else self.stream_fill())
        # both queries' candidate counts of the tile (each at most 4096) in one reduction; the
        # scans run where a path needs them, so no lane count lives across the other path
        return body + ["    int sm_ = __popcll(d_) | (__popcll(db_) << 16);",
                       "    for (int o_ = 32; o_ > 0; o_ >>= 1) sm_ += __shfl_xor(sm_, o_, 64);",
                       "    const int tot_ = sm_ & 0xFFFF, totb_ = sm_ >> 16;"] + self.candidates()

    def tile_loop(self, body: List[str]) -> List[str]:
        """The wavefront's tiles; RS_PIPE 2: unrolled by two over the buffers A and B."""
        def tile(tv: str, cur: str, nxt: str) -> List[str]:
            return ["   {"] + self.subst(body, T=tv, S=cur, O=nxt) + ["   }"]
        if self.f.pipe == 2:
            return ["  for (i64 t = t0; t < t1; t += 2) {"] + tile("t", "A", "B") + \
                ["    if (t + 1 >= t1) break;"] + tile("(t + 1)", "B", "A") + ["  }"]
        return ["  for (i64 t = t0; t < t1; ++t) {"] + tile("t", "A", "A") + ["  }"]

    def epilogue(self) -> List[str]:
        """The block partials (none with a hash table) and the top-K lists.  Adds the top-K
        output slots."""
        aggs, hk, tk, grouped, b = self.aggs, self.hk, self.tk, self.f.grouped, []
        if hk is None and self.f.pair:
            # each query's block partials, folded as in its own launch
            b += ["  {"] + J._flush(aggs, grouped) + ["  }", "  {"] + \
                self.set_b(J._flush(aggs, grouped)) + ["  }"]
        elif hk is None:
            b += J._flush(aggs, grouped)
        if tk is not None:
            b += JH._topk_carry_final(aggs, hk, tk, "  ", self.carry_gen)

            def key_lines(j: int, ind_: str) -> List[str]:
                gk = J._Gen(self.args, self.cols, SPLIT, (f"tkr{j}", f"tkr{j}"), frozenset(), True)
                out: List[str] = []
                for c in hk.cols:
                    J._uload(gk, c.slot, "F", out, ind_)
                out += JH._hash_key_lines(gk, hk, "tkey_l", "_F", ind_)
                out.append(f"{ind_}const u64 tkey_ = tkey_l;")
                return out
            b += JH._topk_flush(aggs, tk, self.args, "wid", key_lines)
        return b


def gen_run_sparse_scan(p: NL.JoinParams, compacts, hk=None, tk=None,
                        cand: tuple = (), pair: bool = False) -> J.Kernel:
    """Phase 2 for 1-bit tags, bit-parallel: the dense per-row scan spends ~20 VALU
    instructions per row (decode, predicate, run index by popcount, tag extract, compaction
    ballot + mbcnt), which bounds it below HBM speed.  Here a wavefront takes 4096-row tiles of
    the left ranges, lane l the 64-row group l of its tile, and works on 64-bit row masks: the
    tag mask (1), the predicate mask (2), and the rows of their AND through an LDS list into the
    walk (3).  The forms, and the ``_BitsScan`` stages a tile takes after ``tag_mask``:

    * streaming (``hs_jit_run_bits_scan``): ``pred_mask``, ``stream_fill``, ``walk``;
    * ``hk`` / ``hk, tk`` (``..._hash`` / ``..._topk``): the same, ``walk`` probing a table /
      keeping a top-K, which ``epilogue`` writes;
    * ``cand`` (``..._cand``): ``candidates`` -> ``cand_loop`` -> ``filter_pass`` with ``append``,
      then ``walk`` (RS_KEEP: through ``consume``);
    * ``cand, pair`` (``..._cand2``): ``candidates`` -> ``pair_union``, or ``cand_loop`` per query
      (``set_b`` for the second).

    The driver is the kernel top to bottom; its order is also the order in which argument slots
    are added (``_BitsScan``), so it is part of the sources' text."""
    s = _BitsScan(p, compacts, hk, tk, cand, pair)
    acc = s.acc_decls()
    bufs = s.loads()        # (before the LDS declarations: RS_LDS sizes its slab by the loads)
    b = acc + s.lds_decls() + s.split() + bufs + s.prologue()
    b += s.tile_loop(s.tile_body())
    b += s.epilogue()
    # (pair form: the second accumulator set and mask put it past the 72 VGPRs of seven waves;
    # left alone the compiler takes 97 - four waves - and bounded to six it spills nine, so it
    # is bounded to five: 96 VGPRs, no scratch.  RS_KEEP: 93 at five; bounded to six it spills 18
    # and to seven 27 - the peak is now in the dense path, whose loop holds the other query's
    # accumulators and mask; the union path alone fits six (73) - so five stays)
    waves = RS_WAVES or (5 if s.f.pair else 0)
    occ = f" __attribute__((amdgpu_waves_per_eu({waves}, {waves})))" if waves else ""
    return J._kernel(s.f.name, s.args, b, (len(s.aggs) * p.num_groups * 32) if s.f.grouped else 0,
                     attrs=occ)


class TwoPhaseLauncher:
    """Both phases lowered once (kernels, tiles, spans, per-tile run windows, the tag bitmap);
    ``launch(p)`` fills the literal slots and queues: bitmap clear, tags, scan, partials fold."""
    __slots__ = ("kt", "ks", "grid_t", "grid_s", "GA", "shmem", "vt", "vs", "compacts", "keep",
                 "tags", "dev", "blocks", "hk", "graph", "gblocks", "tk", "tpl", "match",
                 "launches", "ktp", "tags_b", "tplp", "pblocks", "bblocks", "held", "ksp", "tpls",
                 "sblocks")

    def __init__(self, kt, ks, grid_t, grid_s, GA, shmem, vt, vs, compacts, keep, tags, dev,
                 hk=None, tk=None):
        self.kt, self.ks, self.grid_t, self.grid_s = kt, ks, grid_t, grid_s
        self.GA, self.shmem, self.vt, self.vs = GA, shmem, vt, vs
        self.compacts, self.keep, self.tags, self.dev = compacts, keep, tags, dev
        # literal vector -> (phase-1 block, phase-2 block template): a repeated parameter set
        # re-packs only the per-launch partials pointers
        self.blocks: dict = {}
        # hash-mode phase 2 (a KeyPlan): groups go to a device hash table, no partials
        self.hk = hk
        self.tk = tk          # run top-K mode of the hash walk (hash_agg.TopKPlan)
        # the captured pipeline (graphs.TwoPhaseGraph) and its per-literal-vector blocks
        self.graph = None
        self.gblocks: dict = {}
        # packed argument blocks of the literal-independent slots: a new literal vector patches
        # only its literal slots into copies of these
        self.tpl = None
        # (W, runs, lowered parameters) while phase 1 may still switch to a recorded match
        # (RT2_MATCH): on the launcher's second launch - a lowering that is reused - ``_record``
        self.match = None
        self.launches = 0
        # the pair form of phase 1 (``tags2_pair``) from the lowering, or None; the second tag
        # bitmap and the pair's packed blocks come with the first pair (``launch_pair``)
        self.ktp, self.tags_b, self.tplp = None, None, None
        self.pblocks: dict = {}    # (literal vector A, B) -> pair phase-1 block
        self.bblocks: dict = {}    # literal vector -> phase-2 block reading the second bitmap
        # the pair form of the candidate phase 2 (``cand_pair``) from the lowering, or None: a
        # pair then runs two kernels instead of three; its packed template, and per pair of
        # literal vectors its block, come with the first pair
        self.ksp, self.tpls = None, None
        self.sblocks: dict = {}    # (literal vector A, B) -> pair phase-2 block
        # a submitted query not launched yet (pairing.HeldQuery): it waits for a partner
        self.held = None

    def _record(self) -> None:
        """Switch phase 1 to the recorded-match form: one verifying launch stores each run's
        right row (``record_matches``), later launches read it.  Skipped when the record would
        not fit the device's free memory with a margin; the record counts against the table
        caches' budgets while it lives (``device_cache.track_derived``)."""
        import torch
        from .device_cache import track_derived
        if self.held is not None:       # (a launcher that may still record never holds)
            self.held.release()
        W, nruns, p = self.match
        self.match = None
        need = ((nruns + 63) >> 6) * 64 * 16
        free, _ = torch.cuda.mem_get_info(self.dev)
        free += torch.cuda.memory_reserved(self.dev) - torch.cuda.memory_allocated(self.dev)
        if free < need + (8 << 30):
            return
        try:
            m = record_matches(p, self.compacts, W, self.vt, nruns, self.grid_t, self.dev)
            mode = "copy" if RT2_COPY and copy_ok(p, self.compacts) else "match"
            if mode == "copy":
                held, vals = copy_matches(p, self.compacts, m, self.vt, self.dev)
                # (the match record itself is dropped once the gather ran: stream-ordered frees)
            else:
                held, vals = [m], {"MATCH": m.data_ptr()}
        except torch.OutOfMemoryError:
            return      # an optional copy: the verifying form stays
        for t in held:
            track_derived(t)
        self.kt = J.kernel_for(tags2_shape(p, self.compacts, W, True, mode),
                               lambda: gen_run_tags2(p, self.compacts, W, True, mode))
        self.vt = dict(self.vt, **vals)
        self.keep = self.keep + tuple(held)
        # every packed phase-1 block and the captured pipeline name the verifying kernel
        self.tpl, self.graph = None, None
        self.blocks.clear()
        self.gblocks.clear()
        self.bblocks.clear()
        # the recorded and copy forms have no pair form: from here on ``supports_pair`` is false
        # (nothing is held or paired), and the second bitmap goes
        self.ktp, self.tags_b, self.tplp = None, None, None
        self.pblocks.clear()
        self.ksp, self.tpls = None, None
        self.sblocks.clear()

    def graphable(self) -> bool:
        """Whether one query's launches can be captured: partials out (not the hash mode)."""
        return self.hk is None

    def supports_pair(self) -> bool:
        """Whether two queries can share one phase-1 pass (``launch_pair``): the lowering chose
        the pair-capable kernel, partials out, and no switch to a recorded match is pending."""
        return self.ktp is not None and self.hk is None and self.match is None

    def busy(self) -> bool:
        """Whether the captured pipeline's latest launch has not finished on the device."""
        g = self.graph
        return g is not None and g.busy()

    def _blocks(self, p: NL.JoinParams, key) -> tuple:
        """(phase-1 block, phase-2 block template) of one query's literals."""
        hit = self.blocks.get(key) if key is not None else None
        if hit is None:
            preds = [(k_, p.preds[k_]) for k_ in range(p.npreds)]
            aggs = J.aggs_of(p)
            if self.tpl is None:
                vs0 = dict(self.vs)
                vs0.update({"psum": 0, "pcnt": 0, "pmin": 0, "pmax": 0})
                self.tpl = (bytes(self.kt.args.pack(self.vt, default=0)),
                            bytes(self.ks.args.pack(vs0, default=0)))
            lt: dict = {}
            J.fill_preds_aggs(lt, preds, [], self.compacts)
            ls: dict = {}
            J.fill_preds_aggs(ls, preds, aggs, self.compacts)
            hit = (bytes(self.kt.args.patch(bytearray(self.tpl[0]), lt)),
                   self.ks.args.patch(bytearray(self.tpl[1]), ls))
            if key is not None:
                if len(self.blocks) >= 256:
                    self.blocks.clear()
                self.blocks[key] = hit
        return hit

    def _graph_blocks(self, key, hit) -> tuple:
        """The captured pipeline (made on first use) and ``key``'s blocks for it."""
        import struct
        from .graphs import TwoPhaseGraph, _cbuf
        g = self.graph
        if g is None:
            g = self.graph = TwoPhaseGraph(self.kt, self.ks, self.grid_t, self.grid_s,
                                           self.GA, self.shmem, self.dev)
        gb = self.gblocks.get(key)
        if gb is None:
            bs = bytearray(hit[1])
            a = self.ks.args
            for name, ptr in g.partial_ptrs().items():
                struct.pack_into("<q", bs, a.offset(name), ptr)
            gb = (_cbuf(hit[0]), _cbuf(bs))
            if len(self.gblocks) >= 256:
                self.gblocks.clear()
                self.bblocks.clear()
                self.sblocks.clear()
            self.gblocks[key] = gb
        return g, gb

    def launch_pair(self, p_a: NL.JoinParams, key_a, p_b: NL.JoinParams, key_b) -> tuple:
        """Queue two queries of this lowering that share one phase-1 pass (``supports_pair``):
        the pair kernel tags A into the launcher's bitmap and B into a second one, then each
        query runs its own phase 2, final reduction and result copy, A first - one linear chain,
        captured as one graph (``TwoPhaseGraph.launch_pair``).  With the pair phase 2
        (``ksp``) both queries share that pass too: pair phase 1, pair phase 2, then each
        query's final reduction and result copy.  Returns both queries'
        ``graphs.GraphPending``; each result is bit for bit what ``launch`` gives."""
        import struct
        import torch
        from .graphs import GraphPending, _cbuf
        assert self.supports_pair() and key_a is not None and key_b is not None
        if self.held is not None:
            self.held.release()
        self.launches += 2
        g, gb_a = self._graph_blocks(key_a, self._blocks(p_a, key_a))
        _, gb_b = self._graph_blocks(key_b, self._blocks(p_b, key_b))
        if self.tags_b is None:
            from .device_cache import track_derived
            self.tags_b = torch.empty_like(self.tags)
            track_derived(self.tags_b)
            self.tplp = bytes(self.ktp.args.pack(dict(self.vt, tags_b=self.tags_b.data_ptr()),
                                                 default=0))
        pb = self.pblocks.get((key_a, key_b))
        if pb is None:
            la: dict = {}
            J.fill_preds_aggs(la, [(k_, p_a.preds[k_]) for k_ in range(p_a.npreds)], [],
                              self.compacts)
            lb: dict = {}
            J.fill_preds_aggs(lb, [(k_, p_b.preds[k_]) for k_ in range(p_b.npreds)], [],
                              self.compacts)
            blk = self.ktp.args.patch(bytearray(self.tplp), la)
            pb = _cbuf(self.ktp.args.patch(blk, {n + PAIR_SFX: v for n, v in lb.items()}))
            if len(self.pblocks) >= 256:
                self.pblocks.clear()
            self.pblocks[(key_a, key_b)] = pb
        if self.ksp is not None:
            sp = self.sblocks.get((key_a, key_b))
            if sp is None:
                # the single form's block with the second bitmap, the second literal set and
                # both partial sets patched in
                if self.tpls is None:
                    vs0 = dict(self.vs, tags_b=self.tags_b.data_ptr())
                    vs0.update(g.partial_ptrs())
                    vs0.update(g.partial_ptrs(PAIR_SFX, g.parts_b))
                    self.tpls = bytes(self.ksp.args.pack(vs0, default=0))
                sa_: dict = {}
                J.fill_preds_aggs(sa_, [(k_, p_a.preds[k_]) for k_ in range(p_a.npreds)],
                                  [p_a.aggs[i] for i in range(p_a.naggs)], self.compacts)
                sb_: dict = {}
                J.fill_preds_aggs(sb_, [(k_, p_b.preds[k_]) for k_ in range(p_b.npreds)],
                                  [p_b.aggs[i] for i in range(p_b.naggs)], self.compacts)
                blk = self.ksp.args.patch(bytearray(self.tpls), sa_)
                sp = _cbuf(self.ksp.args.patch(blk, {n + PAIR_SFX: v for n, v in sb_.items()}))
                if len(self.sblocks) >= 256:
                    self.sblocks.clear()
                self.sblocks[(key_a, key_b)] = sp
            ha, hb = g.launch_pair(self.ktp, pb, sp, None, gb_a, self.ksp)
            return GraphPending(g, ha), GraphPending(g, hb)
        sb = self.bblocks.get(key_b)
        if sb is None:
            # B's phase 2 is the single query's block with the second bitmap for ``tags``
            bs = bytearray(gb_b[1].raw)
            struct.pack_into("<q", bs, self.ks.args.offset("tags"), self.tags_b.data_ptr())
            sb = self.bblocks[key_b] = _cbuf(bs)
        ha, hb = g.launch_pair(self.ktp, pb, gb_a[1], sb, gb_a)
        return GraphPending(g, ha), GraphPending(g, hb)

    def launch(self, p: NL.JoinParams, key=None, htab=None, hk=None, graph: bool = False):
        """Queue one query.  Returns the (sum, count, min, max) device outputs, or with
        ``graph`` (and a literal vector ``key``) a ``graphs.GraphPending`` of one replay of the
        captured pipeline."""
        import struct
        if self.held is not None:
            self.held.release()     # submissions of one launcher launch in order
        self.launches += 1
        if self.match is not None and self.launches == 2:
            self._record()
        st = NL.stream_ptr()
        if self.hk is not None:
            preds = [(k_, p.preds[k_]) for k_ in range(p.npreds)]
            vt = dict(self.vt)
            J.fill_preds_aggs(vt, preds, [], self.compacts)
            vs = dict(self.vs)
            vs.update({"psum": 0, "pcnt": 0, "pmin": 0, "pmax": 0})
            J.fill_preds_aggs(vs, preds, J.aggs_of(p), self.compacts)
            vs.update(htab.kernel_values())
            vs.update((hk or self.hk).values())   # this query's key domain
            if self.tk is not None:
                vs.update(self.tk.kernel_values())
                self.tk.used = True
            self.kt.launch(self.grid_t, vt, st, 0)
            self.ks.launch(self.grid_s, vs, st, self.shmem)
            if self.tk is not None:
                self.tk.finish(st)
            return None
        hit = self._blocks(p, key)
        if graph and key is not None and self.graphable():
            from .graphs import GraphPending
            g, gb = self._graph_blocks(key, hit)
            return GraphPending(g, g.launch(*gb))
        # (phase 1 stores every word of every run group: no bitmap clear)
        self.kt.launch_packed(self.grid_t, hit[0], st)
        parts = J._partials(self.grid_s, self.GA, self.dev)
        bs = bytearray(hit[1])
        a = self.ks.args
        for name, t in zip(("psum", "pcnt", "pmin", "pmax"), parts):
            struct.pack_into("<q", bs, a.offset(name), t.data_ptr())
        self.ks.launch_packed(self.grid_s, bs, st, self.shmem)
        return J._final(parts, self.grid_s, self.GA, self.dev)


def lower(p: NL.JoinParams, rstart, rlen, rbucket, roff, compacts, runs, nrows: int,
          cache_spans: bool, hk=None, tk=None, record: bool = False) -> Optional[TwoPhaseLauncher]:
    """The two-phase launcher of a run-keyed merge join, or None when it does not apply.
    ``hk``: group by that hash key plan (left-side key columns only) through the bits scan's
    hash mode (needs 1-bit tags).  None for an empty right side too (nothing to match)."""
    import torch
    if not applies(p) or runs is None or int(roff[-1].item()) <= 0:
        return None
    if hk is not None and (not RS_BITS or tag_width(p) != 1 or _scan_grouped(p) or
                           any(s >= SPLIT for s in hk.slots)):
        return None
    W = tag_width(p)
    NI = RS_ITEMS if RS_ITEMS and 64 % RS_ITEMS == 0 else J._mj_items(True)
    T = J.BLOCK * NI  # noqa: N806
    dev = rstart.device
    max_tiles = nrows // T + 2 * rstart.numel() + 2
    tp, spans = J._join_spans(p, rstart, rlen, rbucket, roff, max_tiles, T, cache_spans, align=NI)
    onebit = W == 1 and not (_scan_grouped(p) and p.group_col >= SPLIT)
    sparse = RS_BITS and onebit
    if tk is not None and hk is None:
        tk = None
    # the pruned pair (``prune_plan``): phase 1 pre-filters by per-run bounds and phase 2 takes
    # the candidate form - always together (the candidate form over unfiltered tags would
    # gather half the table's tail words), and never with the 16-bit-half or recorded phase 1
    prune = prune_plan(p, compacts, W, hk, record) if sparse and not \
        (RT2_LO16 and cache_spans) else ()
    cand = tuple(dict.fromkeys(sl for _, sl, _ in prune))
    if sparse:
        ks = J.kernel_for(sparse_shape(p, compacts, hk, tk, cand),
                          lambda: gen_run_sparse_scan(p, compacts, hk, tk, cand))
    else:
        ks = J.kernel_for(scan_shape(p, compacts, W, NI),
                          lambda: gen_run_scan(p, compacts, W, NI))
    nruns = int(runs.runkeys.numel())
    KW = ((31 + (NI - 1) * W) >> 5) + 1  # noqa: N806
    nwords = max((nruns * W + 31) >> 5, ((nruns + 63) >> 6) * 2 * W)
    tags = torch.empty(nwords + KW + 2, dtype=torch.int32, device=dev)
    frame = J._key32_frame(p, compacts)
    rng = run_ranges(rstart, rlen, rbucket, roff, runs)
    rng_d = torch.from_numpy(rng.reshape(-1).copy() if len(rng) else
                             __import__("numpy").zeros(4, "int64")).to(dev)
    # 32-bit run / right-row indices when both fit (with slack for the gallop's overshoot)
    ix32 = RT2_I32 and nruns < (1 << 31) - (1 << 20) and int(roff[-1].item()) < (1 << 31) - (1 << 20)
    # both keys as 16-bit offsets from 32-element group bases, when both forms exist (else the
    # 32-bit kernel and arguments; a launcher about to switch to a recorded match keeps it too)
    kf = key_forms16(runs, compacts[p.rkey]) if tags2_k16(p, compacts, ix32) and \
        runs is compacts.get(p.lkey) and not (record and RT2_MATCH) else None
    kt = J.kernel_for(tags2_shape(p, compacts, W, ix32, "", prune, kf is not None),
                      lambda: gen_run_tags2(p, compacts, W, ix32, "", prune, kf is not None))
    vt = {"RNG": rng_d.data_ptr(), "NRG": len(rng), "NRUNS": nruns, "tags": tags.data_ptr(),
          "num_groups": p.num_groups, "group_base": p.group_base}
    tr = rng_d
    if kf is not None:
        (vt["LO16"], vt["LG16"]), (vt["RO16"], vt["RG16"]) = \
            ((t.data_ptr() for t in kf[0]), (t.data_ptr() for t in kf[1]))
        tr = (rng_d, kf)
    bnd = []
    for _, sl, mx in prune:
        mn_t, mx_t = run_bounds(runs, compacts[sl])
        vt[f"RMX{sl}" if mx else f"RMN{sl}"] = (mx_t if mx else mn_t).data_ptr()
        bnd += [mn_t, mx_t]
    grid_t = max(1, RT2_WIDE_GRID if tags2_wide(p, compacts, ix32) == 4 else RT2_GRID)
    vt["KLO"], vt["KSP"], vt["KOF"] = frame
    J._fill_cols(vt, p.cols, compacts)
    lo = lo16_keys(p, compacts, W, vt, nruns, int(roff[-1].item()), grid_t, dev) \
        if RT2_LO16 and ix32 and cache_spans and not prune else None
    if lo is not None:
        kt = J.kernel_for(tags2_shape(p, compacts, W, ix32, "lo16"),
                          lambda: gen_run_tags2(p, compacts, W, ix32, "lo16"))
        vt["LL"], vt["RL"] = lo[0].data_ptr(), lo[1].data_ptr()
        tr = (rng_d, lo)
    vs = {"rstart": rstart.data_ptr(), "rlen": rlen.data_ptr(), "tile_prefix": tp.data_ptr(),
          "tags": tags.data_ptr(), "R": rstart.numel(), "nrows": nrows,
          "num_groups": p.num_groups, "group_base": p.group_base}
    J._fill_cols(vs, p.cols, compacts)
    GA = p.naggs * (p.num_groups if p.group_col >= 0 else 1)
    grid_s = max(1, J.SCAN_GRID or NL.lib().hs_scan_grid())
    if sparse:
        from ..ops import kernels as K
        tp64 = K.ranges_to_tiles(rlen + (rstart & 63), 4096)   # 64-aligned 4096-row tiles
        vs["tile_prefix"] = tp64.data_ptr()
        layout = pack_layout(p, compacts, cand)
        pk = packed_tail(layout, compacts) if layout else None
        if pk is not None:
            vs["PK"] = pk.data_ptr()
        # (the candidate form reads no row stream: no 12-bit copy is built for it)
        spans = (spans, tp64, pk, bnd if cand else fill_pack12(vs, p, compacts))
        grid_s = max(1, RS_BITS_GRID)
    if tk is not None:
        tk.bind(grid_s * (J.BLOCK // 64), dev)
    lz = TwoPhaseLauncher(kt, ks, grid_t, grid_s, GA, GA * 32 if _scan_grouped(p) else 0,
                          vt, vs, compacts, (rstart, rlen, rbucket, roff, tp, spans, tr, runs),
                          tags, dev, hk, tk if sparse else None)
    if tags2_pair(p, compacts, W, ix32, "", kf is not None) and lo is None and hk is None:
        # (its module loads, and the second bitmap is made, with the first pair)
        lz.ktp = J.kernel_for(tags2_shape(p, compacts, W, ix32, "", prune, True, True),
                              lambda: gen_run_tags2(p, compacts, W, ix32, "", prune, True, True))
        if sparse and cand_pair(p, compacts, cand, hk, tk):
            lz.ksp = J.kernel_for(sparse_shape(p, compacts, hk, tk, cand, True),
                                  lambda: gen_run_sparse_scan(p, compacts, hk, tk, cand, True))
    if record and RT2_MATCH and ix32:
        # the lowering's own parameters: a later launch's may bind other column slots
        lz.match = (W, nruns, NL.JoinParams.from_buffer_copy(p))
    return lz


def semi_runs_agg(p: NL.JoinParams, rstart, rlen, compacts, runs, nrows: int, words, lo: int,
                  nbits: int):
    """A semi-join probe (``attr in <build-key bitmap>``, GpuBackend._semi_join_agg) over the
    probe key's run form: one bitmap test per run (``hs_run_bitmap_tags``: 1-bit run tags), then
    the bit-parallel phase 2 (``gen_run_sparse_scan``) with the probe's own predicates and
    aggregates - the per-row key read and bitmap test of the plain scan become per-run.  ``p``
    carries the probe side only (slots < SPLIT, ``p.lkey`` = the key slot, ``p.nlp ==
    p.npreds``).  Returns the aggregate outputs (sums, counts, mins, maxs)."""
    import torch
    from ..ops import kernels as K
    dev = rstart.device
    nruns = int(runs.runkeys.numel())
    G = (nruns + 63) >> 6  # noqa: N806
    tags = torch.empty(2 * G + 4, dtype=torch.int32, device=dev)
    st = NL.stream_ptr()
    NL.check(NL.lib().hs_run_bitmap_tags(runs.runkeys.data_ptr(), nruns, int(runs.base) - int(lo),
                                         words.data_ptr(), int(nbits), tags.data_ptr(), st),
             "hs_run_bitmap_tags")
    ks = J.kernel_for(sparse_shape(p, compacts), lambda: gen_run_sparse_scan(p, compacts))
    tp64 = K.ranges_to_tiles(rlen + (rstart & 63), 4096)
    vs = {"rstart": rstart.data_ptr(), "rlen": rlen.data_ptr(), "tile_prefix": tp64.data_ptr(),
          "tags": tags.data_ptr(), "R": rstart.numel(), "nrows": nrows,
          "num_groups": p.num_groups, "group_base": p.group_base}
    J._fill_cols(vs, p.cols, compacts)
    layout = pack_layout(p, compacts)
    pk = packed_tail(layout, compacts) if layout else None
    if pk is not None:
        vs["PK"] = pk.data_ptr()
    p12 = fill_pack12(vs, p, compacts)
    GA = p.naggs * (p.num_groups if p.group_col >= 0 else 1)  # noqa: N806
    grid = max(1, RS_BITS_GRID)
    parts = J._partials(grid, GA, dev)
    vs.update({"psum": parts[0].data_ptr(), "pcnt": parts[1].data_ptr(),
               "pmin": parts[2].data_ptr(), "pmax": parts[3].data_ptr()})
    J.fill_preds_aggs(vs, [(k_, p.preds[k_]) for k_ in range(p.npreds)],
                      J.aggs_of(p), compacts)
    ks.launch(grid, vs, st, GA * 32 if _scan_grouped(p) else 0)
    out = J._final(parts, grid, GA, dev)
    for t in (tags, tp64, pk, *p12):   # used by the queued kernels: keep until they ran
        if t is not None:
            t.record_stream(torch.cuda.current_stream(dev))
    return out
