"""Mutable gallery index, host side (no GPU): ``ops.rows_move`` on CPU tensors (the statement the kernel is held
to) and its refusals; on CPU-"device" indices ``reserve``, appends into reserved space at and over capacity,
``remove`` / ``live``, ``compact`` against ``slice(live)`` in the three layouts through both of its routes, and
``save`` / ``load`` with and without tombstones."""
import pytest
import torch

from fpm import _lib, gallery, ops
from fpm.gallery import GalleryIndex
from fpm.sharded_gallery import ShardedGallery
from test_enroll_keypoints_cpu import special_block
from test_enroll_keypoints_gpu import FIELDS
from test_sharded_gallery_cpu import cpu_index

LAYOUTS = ("f32", "f32+bf16", "bf16+host")
MOVE_CNT = (0, 1, 15, 16, 17, 33)            # both sides of the 16-row band, an empty segment
LABELS = [3, 3, 0, 9, 0, 9, 4]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def move_case(cnts=MOVE_CNT, gap=3):
    """Source rows with specials (NaN, +-inf, -0, subnormals) inside the segments -- ``special_block``'s first row
    as the first row of the segments of 1, 15 and 17 rows, its last row as the last row of those of 16 and 33,
    a NaN in the 15-row one -- and the segments in a scrambled destination order with ``gap`` rows between them
    -> (src32, src_off, dst_off, cnt, dst_rows)."""
    cnt = torch.tensor(cnts, dtype=torch.int64)
    src_off = torch.cat([torch.zeros(1, dtype=torch.int64), (cnt + 2).cumsum(0)[:-1]]) + 1
    src = special_block(int(src_off[-1] + cnt[-1]) + 4)
    for k in (1, 2, 4):
        src[int(src_off[k])] = src[0]
    for k in (3, 5):
        src[int(src_off[k] + cnt[k]) - 1] = src[-1]
    src[int(src_off[2]), 25] = float("nan")
    order = torch.tensor([3, 0, 5, 1, 4, 2][:len(cnts)]) if len(cnts) == 6 else torch.arange(len(cnts))
    dst_off = torch.zeros(len(cnts), dtype=torch.int64)
    at = 2
    for k in order.tolist():
        dst_off[k] = at
        at += int(cnt[k]) + gap
    return src, src_off, dst_off, cnt, at + 1


def moved_specials(src, src_off, cnt):
    """Assert that the rows the segments move hold NaN, +inf, -inf, -0 and (fp32) a subnormal, so that "preserved
    as bits" is about something."""
    rows = torch.cat([src[s:s + k] for s, k in zip(src_off.tolist(), cnt.tolist())])
    bits = rows.float().contiguous().view(torch.int32)          # bf16 -> fp32 is exact
    assert bool(torch.isnan(rows).any()) and bool((rows == float("inf")).any()) and bool((rows == float("-inf")).any())
    assert bool((bits == -(1 << 31)).any())                     # -0
    if rows.dtype == torch.float32:
        assert bool(((bits & 0x7F800000) == 0).logical_and((bits & 0x007FFFFF) != 0).any())


def move_statement(src, src_off, dst_off, cnt, dst):
    """The copy, a row at a time."""
    for s, d, k in zip(src_off.tolist(), dst_off.tolist(), cnt.tolist()):
        for r in range(k):
            dst[d + r] = src[s + r]
    return dst


# --------------------------------------------------------------------------------------- rows_move
@pytest.mark.parametrize("which", ["f32", "b16", "both"])
def test_rows_move_host(which):
    src, so, do, cnt, rows = move_case()
    s16 = src.to(torch.bfloat16)
    s16.view(torch.int16)[int(so[3]), 7] = 0x7FC1                  # a NaN with a payload: copied as bits
    moved_specials(src, so, cnt)
    moved_specials(s16, so, cnt)
    d32 = torch.full((rows, 768), float("nan")) if which != "b16" else None
    d16 = torch.full((rows, 768), float("nan"), dtype=torch.bfloat16) if which != "f32" else None
    got = ops.rows_move(so, do, cnt, src32=None if d32 is None else src, dst32=d32, src16=None if d16 is None else s16,
                        dst16=d16)
    assert got[0] is d32 and got[1] is d16
    written = torch.zeros(rows, dtype=torch.bool)
    for d, k in zip(do.tolist(), cnt.tolist()):
        written[d:d + k] = True
    for dst, s in ((d32, src), (d16, s16)):
        if dst is None:
            continue
        want = move_statement(s, so, do, cnt, torch.full_like(dst, float("nan")))
        assert torch.equal(_bits(dst), _bits(want))
        assert bool(torch.isnan(dst[~written]).all())              # rows outside the destination ranges keep the fill
    assert int(written.sum()) == int(cnt.sum())


def test_rows_move_one_segment_and_same_tensor():
    """K = 1; one tensor as source and destination with disjoint ranges (how an index is compacted in place)."""
    src, _, _, _, _ = move_case()
    out = torch.full((40, 768), float("nan"))
    one = lambda v: torch.tensor([v], dtype=torch.int64)
    moved_specials(src, one(5), one(17))                                         # rows 5 .. 21: the specials of row 6
    ops.rows_move(one(5), one(20), one(17), src32=src, dst32=out)
    assert torch.equal(_bits(out[20:37]), _bits(src[5:22])) and bool(torch.isnan(out[:20]).all())
    buf = src.clone()
    so, do, cnt = torch.tensor([6, 38, 60]), torch.tensor([15, 24, 50]), torch.tensor([9, 12, 10])
    moved_specials(src, so, cnt)                                                 # the special rows 6, 38 and 41
    ops.rows_move(so, do, cnt, src32=buf, dst32=buf)
    assert torch.equal(_bits(buf), _bits(move_statement(src, so, do, cnt, src.clone())))
    b16 = src.to(torch.bfloat16)
    want16 = move_statement(b16.clone(), so, do, cnt, b16.clone())
    moved_specials(b16, so, cnt)
    ops.rows_move(so, do, cnt, src32=buf, dst32=buf, src16=b16, dst16=b16)       # the ranges are disjoint again
    assert torch.equal(_bits(b16), _bits(want16))
    ops.rows_move(so[:0], do[:0], cnt[:0], src32=buf, dst32=buf)                 # no segment: nothing happens


def test_rows_move_refusals(monkeypatch):
    def trap(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "call", trap)
    src, so, do, cnt, rows = move_case()
    dst = torch.zeros(rows, 768)
    s16, d16 = src.to(torch.bfloat16), dst.to(torch.bfloat16)
    ops.rows_move(so, do, cnt, src32=src, dst32=dst, src16=s16, dst16=d16)
    R = _lib.FpmError
    same = src.clone()
    t = lambda *v: torch.tensor(v, dtype=torch.int64)
    with pytest.raises(R, match="a destination range meets a source range"):
        ops.rows_move(t(10), t(5), t(8), src32=same, dst32=same)                 # [5, 13) meets [10, 18)
    with pytest.raises(R, match="a destination range meets a source range"):
        ops.rows_move(t(10, 40), t(60, 17), t(8, 5), src32=same, dst32=same)     # segment 1 writes segment 0's source
    with pytest.raises(R, match="a destination range meets a source range"):
        ops.rows_move(t(10), t(10), t(1), src32=same, dst32=same)
    ops.rows_move(t(10), t(2), t(8), src32=same, dst32=same)                     # [2, 10) ends where [10, 18) begins
    with pytest.raises(R, match="share memory without being the same rows"):
        ops.rows_move(t(10), t(0), t(8), src32=same, dst32=same[1:])
    with pytest.raises(R, match="two destination ranges meet"):
        ops.rows_move(t(0, 20), t(5, 9), t(5, 5), src32=src, dst32=dst)
    with pytest.raises(R, match="a source range outside"):
        ops.rows_move(t(src.shape[0] - 3), t(0), t(4), src32=src, dst32=dst)
    with pytest.raises(R, match="a source range outside"):
        ops.rows_move(t(-1), t(0), t(4), src32=src, dst32=dst)
    with pytest.raises(R, match="a destination range outside"):
        ops.rows_move(t(0), t(rows - 3), t(4), src32=src, dst32=dst)
    with pytest.raises(R, match="a destination range outside"):                  # the shorter of the two destinations
        ops.rows_move(t(0), t(rows - 3), t(3), src32=src, dst32=dst, src16=s16, dst16=d16[:-1])
    with pytest.raises(R, match="a negative row count"):
        ops.rows_move(t(0), t(0), t(-1), src32=src, dst32=dst)
    with pytest.raises(R, match="one of each per segment"):
        ops.rows_move(so, do, cnt[:-1], src32=src, dst32=dst)
    with pytest.raises(R, match="one of each per segment"):
        ops.rows_move(so[:-1], do, cnt, src32=src, dst32=dst)
    with pytest.raises(R, match="host copies"):
        ops.rows_move(so, do, cnt, src32=src, dst32=dst, cnt_host=cnt[:-1])
    with pytest.raises(R, match="cnt must be a int64 tensor"):
        ops.rows_move(so, do, cnt.int(), src32=src, dst32=dst)
    with pytest.raises(R, match="src_off must be a int64 tensor"):
        ops.rows_move(so.int(), do, cnt, src32=src, dst32=dst)
    with pytest.raises(R, match="dst_off must be a contiguous 1-d tensor"):
        ops.rows_move(so, torch.stack([do, do], 1)[:, 0], cnt, src32=src, dst32=dst)
    with pytest.raises(R, match="src32 must be contiguous fp32 rows"):
        ops.rows_move(so, do, cnt, src32=src.double(), dst32=dst)
    with pytest.raises(R, match="dst32 must be contiguous fp32 rows"):
        ops.rows_move(so, do, cnt, src32=src, dst32=d16)
    with pytest.raises(R, match="src16 must be contiguous bf16 rows"):
        ops.rows_move(so, do, cnt, src16=s16.to(torch.float16), dst16=d16)
    with pytest.raises(R, match="dst32 must be contiguous fp32 rows"):
        ops.rows_move(so, do, cnt, src32=src, dst32=torch.zeros(rows, 1536)[:, ::2])
    with pytest.raises(R, match="src32 must be contiguous fp32 rows"):
        ops.rows_move(so, do, cnt, src32=torch.zeros(src.shape[0], 1536)[:, ::2], dst32=dst)
    with pytest.raises(R, match="src32 goes with dst32"):
        ops.rows_move(so, do, cnt, src32=src, dst16=d16)
    with pytest.raises(R, match="give the fp32 rows"):
        ops.rows_move(so, do, cnt)
    with pytest.raises(R, match="at most 65535 segments"):
        big = torch.zeros(65536, dtype=torch.int64)
        ops.rows_move(big, big, big, src32=src, dst32=dst)


# ------------------------------------------------------------------------------------ index storage
def same_fields(a, b, what="", pack_gen=True):
    """Every field of FIELDS plus ``subject``, dtype and bits (``pack_gen``: and the weight-pack generation, which
    two enrolments at different times need not share)."""
    for k in FIELDS + ("subject",):
        u, v = getattr(a, k), getattr(b, k)
        if isinstance(u, torch.Tensor):
            assert isinstance(v, torch.Tensor) and u.dtype == v.dtype and u.device == v.device, (what, k)
            assert tuple(u.shape) == tuple(v.shape) and torch.equal(u.contiguous().view(torch.uint8),
                                                                     v.contiguous().view(torch.uint8)), (what, k)
        else:
            assert u == v, (what, k)
    assert a.layout == b.layout and a.G == b.G and torch.equal(a.row_off.cpu(), a.row_off_host)
    assert not pack_gen or a._pack_gen == b._pack_gen


def snapshot(index):
    """The index's fields as copies, its counters and the views' addresses."""
    return ({k: (getattr(index, k).clone() if isinstance(getattr(index, k), torch.Tensor) else getattr(index, k))
             for k in FIELDS + ("subject",)}, index.generation, index.used, index.removed.clone(),
            {k: getattr(index, k).data_ptr() for k in ("y", "src", "w", "row_off")})


def unchanged(index, snap):
    fields, gen, used, removed, ptrs = snap
    for k, v in fields.items():
        u = getattr(index, k)
        if isinstance(v, torch.Tensor):
            assert u.dtype == v.dtype and torch.equal(u.view(torch.uint8), v.view(torch.uint8)), k
        else:
            assert u == v, k
    assert index.generation == gen and index.used == used and torch.equal(index.removed, removed)
    assert ptrs == {k: getattr(index, k).data_ptr() for k in ptrs}


@pytest.mark.parametrize("layout", LAYOUTS)
def test_reserve_keeps_every_field(layout):
    parent = cpu_index(layout, labels=LABELS)
    G, R, E = parent.used
    assert parent.capacity is None and parent.generation == 0
    idx = parent.reserve(G + 3, R + 10, E + 12)
    same_fields(idx, parent)
    assert idx.capacity == (G + 3, R + 10, E + 12) and idx.used == (G, R, E) and idx.generation == 0
    assert idx.y.data_ptr() != parent.y.data_ptr() and idx.y.is_contiguous() and idx.row_off.is_contiguous()
    rows = (R + 10) * 768
    assert idx.host_nbytes() == (4 * rows if layout == "bf16+host" else 0)
    assert idx.nbytes() == ({"f32": 4, "f32+bf16": 6, "bf16+host": 2}[layout] * rows + (R + 10) * 8 + (E + 12) * 16
                            + (G + 3) * 2048 + (G + 4) * 8)
    assert cpu_index(layout).reserve(G, R).capacity == (G, R, 6 * R)          # the default: 6 edges per row
    for bad in ((G - 1, R, E), (G, R - 1, E), (G, R, E - 1)):
        with pytest.raises(_lib.FpmError, match="capacity .* below"):
            parent.reserve(*bad)


def _addition(layout, G=2, labels=(7, 3), seed=8):
    return cpu_index(layout, G=G, labels=list(labels), seed=seed)


def append(index, add):
    """The entries of ``add`` appended the way the enrolment loops do it: the refusals, the rows written past
    ``used``, then the small arrays and the commit."""
    R = int(add.y.shape[0])
    at = index._begin_append("append", add.G, R, add.subject, add.P is not None)
    index._store["y"][at[1]:at[1] + R].copy_(add.y)
    if add.y16 is not None:
        index._store["y16"][at[1]:at[1] + R].copy_(add.y16)
    return index._finish_append("append", at, add.n, add.w, add.P, add.src, add.dst, add.pseudo,
                                add.edge_off[1:] - add.edge_off[:-1], add.subject)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_append_at_and_over_capacity(layout):
    """The two ends of the append path ``Net.enroll_into`` runs (``append`` above), without a net: capacity exactly full is accepted; one entry, one row and one edge too many are each refused, and the
    index is unchanged field by field."""
    parent, add = cpu_index(layout, labels=LABELS), _addition(layout)
    G, R, E = parent.used
    g, r, e = add.used
    assert e > 0
    full = parent.reserve(G + g, R + r, E + e)
    new = append(full, add)
    assert new.tolist() == [G, G + 1] and full.used == full.capacity == (G + g, R + r, E + e)
    assert full.generation == 1
    same_fields(full.slice(torch.arange(G)), parent)
    same_fields(full.slice(new), add)
    assert torch.equal(full.row_off_host[G:] - R, add.row_off_host) and torch.equal(full.edge_off[G:] - E, add.edge_off)
    assert full.subject.tolist() == LABELS + [7, 3]
    for cap, why in (((G + g - 1, R + r, E + e), "pass the index's capacity"),
                     ((G + g, R + r - 1, E + e), "pass the index's capacity"),
                     ((G + g, R + r, E + e - 1), "edges pass the index's capacity")):
        idx = parent.reserve(*cap)
        snap = snapshot(idx)
        with pytest.raises(_lib.FpmError, match=why):
            append(idx, add)
        unchanged(idx, snap)
        same_fields(idx, parent)
    idx = parent.reserve(G + g, R + r, E + e)
    snap = snapshot(idx)
    with pytest.raises(_lib.FpmError, match="has no capacity"):
        append(parent, add)
    with pytest.raises(_lib.FpmError, match="the index has subject labels, the call gives none"):
        append(idx, cpu_index(layout, G=2, seed=8))
    with pytest.raises(_lib.FpmError, match="the index has no subject labels, the call gives subjects"):
        append(cpu_index(layout).reserve(G + g, R + r, E + e), add)
    noP = _addition(layout)
    noP.P = None
    with pytest.raises(_lib.FpmError, match="keeps keypoints P, the new graphs carry none"):
        append(idx, noP)
    unchanged(idx, snap)


def test_append_drops_the_caches():
    idx = cpu_index("bf16+host", labels=LABELS).reserve(12, 60, 80)
    idx.subject_groups()
    idx.fetch(torch.tensor([1, 2]))
    buf = idx._stage[1]
    assert idx._groups is not None
    append(idx, _addition("bf16+host"))
    assert idx._groups is None and idx._sel is None and idx._stage[1] is buf and idx._stage[0].numel() == 0
    ys, off_d, off_h = idx.fetch(torch.tensor([1, 2]))                           # the key went: fetched again
    assert torch.equal(ys, torch.cat([idx.y[int(idx.row_off_host[g]):int(idx.row_off_host[g + 1])] for g in (1, 2)]))


# --------------------------------------------------------------------------------- remove and live
def test_remove_live_and_refusals():
    idx = cpu_index("f32", labels=LABELS)
    G = idx.G
    assert idx.live.tolist() == list(range(G)) and not idx.tombstones and not bool(idx.removed.any())
    idx.remove([2, 5])
    assert idx.G == G and idx.live.tolist() == [0, 1, 3, 4, 6] and idx.live.dtype == torch.int64
    assert idx.removed.tolist() == [False, False, True, False, False, True, False] and idx.generation == 1
    assert gallery._select_host(idx, None, "q") is idx.live
    R = _lib.FpmError
    snap = snapshot(idx)
    with pytest.raises(R, match="entry 5 was removed already"):
        idx.remove([0, 5])
    with pytest.raises(R, match="named twice"):
        idx.remove([0, 0])
    for bad in ([G], [-1], []):
        with pytest.raises(R, match=r"must name entries in \[0, 7\)"):
            idx.remove(bad)
    with pytest.raises(R, match="the last live entry"):
        idx.remove([0, 1, 3, 4, 6])
    unchanged(idx, snap)
    # every way to name an entry refuses a dead slot
    with pytest.raises(R, match="identify: entry 2 was removed"):
        gallery._select_host(idx, [0, 2], "identify")
    with pytest.raises(R, match="GalleryIndex.slice: entry 5 was removed"):
        idx.slice(torch.tensor([4, 5]))
    with pytest.raises(R, match="subject_groups: entry 2 was removed"):
        idx.subject_groups([2])
    host = cpu_index("bf16+host")
    host.remove([3])
    with pytest.raises(R, match="GalleryIndex.fetch: entry 3 was removed"):
        host.fetch(torch.tensor([3]))
    # "all entries" are the live ones: the groups of select=None are those of select=live
    twin = cpu_index("f32", labels=LABELS)
    a, b = idx.subject_groups(), twin.subject_groups(idx.live)
    for k in ("labels", "off", "pos", "group"):
        assert torch.equal(a[k], b[k]), k
    idx.set_subjects(list(range(G)))                                             # still G labels, one per slot
    assert idx.subject_groups()["labels"].tolist() == [0, 1, 3, 4, 6]
    idx.remove([0, 1, 3, 4])
    assert idx.live.tolist() == [6]
    with pytest.raises(R, match="a shard has removed entries"):
        ShardedGallery([idx])


def test_sharded_gallery_refuses_a_changed_shard():
    a, b = cpu_index("f32", seed=1).reserve(10, 60, 80), cpu_index("f32", seed=2)
    sg = ShardedGallery([a, b])
    sg._check_unchanged("identify")
    append(a, cpu_index("f32", G=2, seed=3))
    with pytest.raises(_lib.FpmError, match="shard 0 has changed since this ShardedGallery was built"):
        sg._check_unchanged("identify")
    ShardedGallery([a, b])._check_unchanged("identify")


# ----------------------------------------------------------------------------------------- compact
REMOVALS = {"first": [0], "last": [6], "middle": [2, 3, 5], "all-but-one": [0, 1, 2, 3, 5, 6]}


@pytest.mark.parametrize("which", sorted(REMOVALS))
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("reserved", [False, True])
def test_compact_equals_slice_of_live(layout, which, reserved):
    idx, twin = cpu_index(layout, labels=LABELS), cpu_index(layout, labels=LABELS)
    if reserved:
        idx = idx.reserve(9, 50, 60)
    gone = REMOVALS[which]
    idx.remove(gone)
    live = idx.live.clone()
    ptr, cap, gen = idx.y.data_ptr(), idx.capacity if reserved else idx.used, idx.generation
    big = int(twin.n.max())
    new_of_old = idx.compact(stage_rows=big)
    want = twin.slice(live)
    same_fields(idx, want, which)
    assert new_of_old.dtype == torch.int64 and new_of_old[live].tolist() == list(range(len(live)))
    assert bool((new_of_old[torch.tensor(gone)] == -1).all())
    assert idx.y.data_ptr() == ptr and idx.capacity == cap and idx.generation == gen + 1      # the same storage
    assert not idx.tombstones and idx.live.tolist() == list(range(len(live)))
    routes = idx.last_compact
    moved = sum(int(twin.n[e]) for e in live.tolist() if int(new_of_old[e]) != e)
    assert routes["rows"] == moved and routes["launches"] == routes["direct"] + 2 * routes["staged"]
    if which == "last":
        assert routes["launches"] == 0                                           # nothing moves
    # cpu_index's counts are n = [2, 5, 3, 1, 2, 1, 3] and stage_rows = 5: several blocks, and over the removals
    # both routes.  Without entry 0 every block moves up by 2 rows, fewer than it holds: onto rows it still
    # occupies, through the stage; so does the one block of entries 4 and 6 without 2, 3 and 5 (rows 11 .. 17 to
    # 7 .. 12).  With entry 4 alone left, it lands before its own start: one launch, storage to storage.
    if which == "first":
        assert routes["staged"] == 4 and routes["direct"] == 0
    if which == "middle":
        assert routes["staged"] == 1 and routes["direct"] == 0
    if which == "all-but-one":
        assert routes["direct"] == 1 and routes["staged"] == 0
    # the compacted index goes on: append and remove again
    if reserved:
        append(idx, _addition(layout))
        same_fields(idx.slice(torch.arange(len(live))), want)
        same_fields(idx.slice(torch.arange(len(live), len(live) + 2)), _addition(layout))


def test_compact_routes_and_stage():
    """Default stage: one block; a stage below the largest entry to move is refused and nothing changes."""
    idx, twin = cpu_index("f32+bf16", G=40, seed=3), cpu_index("f32+bf16", G=40, seed=3)
    gone = list(range(1, 40, 4))
    idx.remove(gone)
    live = idx.live.clone()
    snap = snapshot(idx)
    with pytest.raises(_lib.FpmError, match="stage_rows = 0 below the largest entry"):
        idx.compact(stage_rows=0)
    unchanged(idx, snap)
    idx.compact()
    assert idx.last_compact["direct"] + idx.last_compact["staged"] == 1
    same_fields(idx, twin.slice(live))
    both = cpu_index("f32", G=40, seed=3)
    both.remove(gone)
    both.compact(stage_rows=7)
    assert both.last_compact["direct"] >= 1 and both.last_compact["staged"] >= 1
    same_fields(both, cpu_index("f32", G=40, seed=3).slice(live))
    none = cpu_index("f32")
    assert none.compact().tolist() == list(range(none.G)) and none.generation == 0 and none.capacity is None


def test_compact_host_rows_in_pieces(monkeypatch):
    """The host rows of "bf16+host" move a run of adjacent entries at a time; with pieces no longer than the
    run's shift no temporary is taken, with longer ones (the default, at these sizes) each piece is."""
    gone = list(range(1, 40, 4)) + [2]
    want = cpu_index("bf16+host", G=40, seed=3).slice(torch.tensor([e for e in range(40) if e not in gone]))
    for rows in (1, gallery.COMPACT_HOST_ROWS):
        monkeypatch.setattr(gallery, "COMPACT_HOST_ROWS", rows)
        idx = cpu_index("bf16+host", G=40, seed=3)
        idx.remove(gone)
        idx.compact()
        same_fields(idx, want)
        assert idx.capacity == (40, int(cpu_index("bf16+host", G=40, seed=3).y.shape[0]), idx.capacity[2])


# ----------------------------------------------------------------------------------- save and load
@pytest.mark.parametrize("layout", LAYOUTS)
def test_save_load(layout, tmp_path):
    plain = cpu_index(layout, labels=LABELS)
    G, R, E = plain.used
    plain.save(tmp_path / "plain.pt")
    roomy = plain.reserve(G + 4, R + 9, E + 9)
    roomy.save(tmp_path / "roomy.pt")
    a = torch.load(tmp_path / "plain.pt", weights_only=True)
    b = torch.load(tmp_path / "roomy.pt", weights_only=True)
    assert list(a) == list(b) and a["format"] == b["format"] == (1 if layout == "f32" else 2) and "removed" not in b
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
            assert b[k].untyped_storage().nbytes() == a[k].untyped_storage().nbytes(), k     # the used part alone
        else:
            assert a[k] == b[k], k
    same_fields(GalleryIndex.load(tmp_path / "roomy.pt", "cpu"), plain)
    back = GalleryIndex.load(tmp_path / "roomy.pt", "cpu", capacity=(G + 2, R + 8, E + 6))
    same_fields(back, plain)
    assert back.capacity == (G + 2, R + 8, E + 6) and back.generation == 0
    append(back, _addition(layout))
    with pytest.raises(_lib.FpmError, match="capacity .* below"):
        GalleryIndex.load(tmp_path / "roomy.pt", "cpu", capacity=(G - 1, R, E))
    # tombstones: format 3 carries the table
    roomy.remove([1, 4])
    roomy.save(tmp_path / "dead.pt")
    d = torch.load(tmp_path / "dead.pt", weights_only=True)
    assert d["format"] == 3 and d["removed"].tolist() == roomy.removed.tolist() and d["layout"] == layout
    for cap in (None, (G + 1, R + 1, E + 1)):
        back = GalleryIndex.load(tmp_path / "dead.pt", "cpu", capacity=cap)
        same_fields(back, plain)
        assert back.live.tolist() == [0, 2, 3, 5, 6] and back.tombstones
        back.compact()
        same_fields(back, plain.slice(torch.tensor([0, 2, 3, 5, 6])))
    roomy.compact()
    roomy.save(tmp_path / "clean.pt")
    assert torch.load(tmp_path / "clean.pt", weights_only=True)["format"] == (1 if layout == "f32" else 2)
