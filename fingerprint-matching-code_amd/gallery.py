"""Enrolled gallery for 1:N identification: templates enrolled once, probes searched many times.

SplineConv is the matcher's per-graph stage: its output rows depend on the graph alone, not on the
partner graph of a pair (``Net._probe_rows`` uses the same fact for the probe side).  ``Net.enroll``
runs the two SplineConv layers over the gallery once and keeps the fp32 output rows in a
``GalleryIndex``; ``Net.identify`` then runs the probe x gallery forward with side 1's operand rows
gathered from the index (``fpm_rows_gather_scale``) instead of recomputed -- the same values, so
every output equals ``net.run(DeviceBatch.from_probe_gallery(probe, gallery))`` bit for bit -- and
ranks the pair scores on the device (``fpm_rank_topk``).

``identify(shortlist=M)`` puts a coarse pass in front: ``coarse_scores`` (one fused kernel per pair,
``fpm_coarse_score``: bf16 vertex affinity, Sinkhorn and <P, Kp> without the block leaving the CU;
``coarse="wide"`` / ``"auto"``: ``fpm_coarse_score_wide`` for boxes of up to 256 keypoints;
``"stream"`` / ``"any"``: ``fpm_coarse_score_stream`` for every box the matcher takes, up to 600)
over the selected entries, ``fpm_rank_select`` to the M best, and the forward above over those alone.

Size of an index: 768 fp32 channels = 3 KB per keypoint (0.39 MB per template at n = 128, 0.4 GB per
1024 such templates), plus the graph's edges (12 B each, ~6 per keypoint) and 2 KB of global feature.

Layouts (``enroll(layout=...)``): the coarse score is defined on b = bf16(y_g), so a bf16 copy of the
rows, rounded once at enrolment (``y16``), serves the coarse kernels with the same bits at half the
bytes ("f32+bf16": the copy beside the fp32 rows).  The exact forward needs fp32 rows only for the
M <= 1024 shortlisted entries, so "bf16+host" keeps them in pinned host memory and ``fetch``es those M
entries per query (``fpm_rows_fetch``): 1.5 KB per keypoint on the device, twice the gallery per GPU,
and every output of ``identify(shortlist=M)`` the same bits as from the "f32" layout.  "fp8+host" holds the
device rows as e4m3 bytes with one power-of-two fp32 scale per row (``y8``, ``s8``; ``ops.rows_quant8`` at
enrolment): 772 B per keypoint.  The coarse operand is then b = bf16(float(y8) * s8), which is exact, so the coarse
score is the bf16 kernels' on those rows (the _rows8 entry points); it differs from the other layouts' only in
which entries a shortlist keeps, and every exact output of an entry is the same bits as from any layout.

Probe sets (``Net.identify_many``, ``coarse_scores_many``, ``match_pairs``): the probes enrolled like a
gallery, so that many probes are searched at once over (probe, entry) pair lists: the coarse kernels'
pair-list instantiations (``ops.coarse_pairs``) score all pairs in bounded launches, and the exact
forward runs in groups of probes (``probe_groups``) on batches whose two sides are both gathered from
cached rows (``pair_batch``).  Every score and output is the bits of the one-probe path's for the same
pair and padded box.

From keypoints (``Net.enroll_keypoints``, ``enroll_images``, ``probe_graphs``): ``enroll`` reads host
graph dicts; ``_enroll_device`` takes padded keypoints and features where they are, builds each
sub-batch's graphs on the device (``graphs.build_graph_batch``) and packs its ragged output rows -- fp32,
bf16 or both -- into an index allocated once (``fpm_rows_pack``, one launch per sub-batch): every field
equals ``enroll``'s on the same graphs.  Probe dicts of device tensors are staged by the query calls as
they are (``_probe_tensors``).

Subjects (``enroll*(subjects=...)``, ``GalleryIndex.set_subjects``, ``identify`` / ``identify_many(by="subject")``):
an entry is one impression, a subject (a finger) has several.  The index keeps one label per entry and
makes a selection's CSR group tables on the host (``subject_groups``); the queries fuse scores per subject
on the device (``ops.group_scores``: max, or a mean in a fixed order) between the coarse scores and
``rank_select`` -- the shortlist then counts subjects -- and between the exact scores and ``rank_topk``.
The exact forward still runs over plain entry lists, so every per-pair output is the entry-level call's.

Query stages: ``identify`` and ``identify_many`` are the same sequence for every form (one probe or a probe
set, entries or subjects, with or without a shortlist): the checks (``_check_eager``, ``_check_query``;
``_check_many``), the coarse scores (``coarse_scores`` / ``coarse_scores_many``), the shortlist stage
(``_shortlist``: the file's one ``rank_select`` and its one coarse fuse; ``_all_lists`` without a shortlist), the
exact stage (one probe: the plain ``identify(select=...)`` per probe, the shared side 0 with the probe's
SplineConv live; a probe set: ``_exact_many``, groups of ragged pair lists with both sides cached), the ranking
(``_entry_ranking`` or ``_subject_ranking``), the open-set stage when asked for (``_open_set``) and ``_attach``,
which puts the result keys on the dicts.  The stages take and return tensors and run on CPU tensors as they are;
the device contexts stay in the callers.

Open set (``top_r``, ``normalize="cohort"``, ``threshold``; all off by default, and then nothing above changes):
``top_r`` makes the exact-stage fuse the mean of a subject's r best impressions (``ops.group_topr``);
``_open_set`` takes ``ops.rank_select`` of the row the ranking ranked and ``ops.cohort_decide``: z-scores of the
top k against the next-best candidates of the same list, ``accept`` per rank and one ``match`` per probe.

Several GPUs (``sharded_gallery.ShardedGallery``): ``GalleryIndex.slice`` cuts an index into parts; ``identify``
over a sharded gallery branches to ``identify_sharded`` there, which runs the stages above per shard and merges the
shards' shortlists (``ops.topk_merge``); ``probe_batch(pad_to=...)`` lays a shard's part of a list out in the whole
list's box, so that the parts' outputs are the one-index forward's.

Prescreen (``identify`` / ``identify_many(shortlist=M, prescreen=K)``; opt-in, and without it nothing above changes):
an index may hold one pooled bf16 descriptor per entry (``GalleryIndex.desc``: ``enroll*(descriptors=True)``,
``add_descriptors``; ``ops.rows_pool``).  ``_prescreen`` scores the probes' descriptors against the selection's
(``ops.desc_score``) and keeps each probe's K best entries in entry order (``ops.rank_keep``); the coarse pass then runs
over each probe's own list (``_coarse_one``, or ``_coarse_many`` over the Q x K pair lists) and ``_shortlist`` maps its
positions through that list.

A mutable index (``GalleryIndex.reserve``, ``enroll*(capacity=...)``; ``Net.enroll_into`` and its keypoint and image
forms; ``remove``, ``compact``): storage with capacity, of which the public fields are prefix views, re-made by the one
``_commit``; appends write past ``used`` and commit at the end; ``remove`` sets tombstones and every query then runs
over ``live`` (``_select_host`` defines "all entries"); ``compact`` moves the live rows to the front inside the same
storage with ``ops.rows_move``, in ascending blocks, storage to storage where a block's destination ends before its
source begins and through a staging buffer otherwise.  No mutation allocates or frees row storage, and no launch reads
rows that it writes.
"""
import contextlib
import hashlib
from collections import namedtuple

import numpy as np
import torch

from . import config as C
from . import ops
from ._lib import FpmError
from .batch import DeviceBatch, ORDER_MIN_NMAX, ORDER_ON, hilbert_order
from .model import _CachedSide

SCORES = ("cls_prob", "cls_logits", "k_prob")
FORMAT = 1                    # a saved "f32" index; the other layouts write FORMAT_LAYOUTS
FORMAT_LAYOUTS = 2
FORMAT_TOMBSTONES = 3         # any layout, with the table ``removed`` (an index saved with removed slots)
FORMAT_FP8 = 4                # the "fp8+host" layout: ``y8`` and ``s8`` for ``y16``; ``removed`` with tombstones
FORMAT_DESC = 5               # any layout (its own row fields), with ``desc``; ``removed`` with tombstones
FORMATS = (FORMAT, FORMAT_LAYOUTS, FORMAT_TOMBSTONES, FORMAT_FP8, FORMAT_DESC)
LAYOUTS = ("f32", "f32+bf16", "bf16+host", "fp8+host")
HOST_LAYOUTS = ("bf16+host", "fp8+host")      # the fp32 rows in (pinned) host memory: ``fetch``
BF16_LAYOUTS = ("f32+bf16", "bf16+host")      # a bf16 copy of the rows on the device: ``y16``
FP8_LAYOUT = "fp8+host"                       # e4m3 rows and their scales on the device: ``y8``, ``s8``
ROW_BYTES_FP8 = C.NODE_FEATURE_DIM + 4        # device bytes per keypoint of the fp8 layout's rows
ROW_BYTES = 4 * C.NODE_FEATURE_DIM
# the fp32 rows one ``GalleryIndex.fetch`` stages on the device at most: those of the largest shortlist
# the API allows (1.89 GB)
FETCH_MAX_BYTES = ops.RANK_SELECT_KMAX * ops.COARSE_STREAM_NMAX * ROW_BYTES
# the rows of the device buffer ``GalleryIndex.compact`` stages blocks in whose destination meets their source
COMPACT_STAGE_BYTES = 64 << 20
DESC_STAGE_BYTES = 64 << 20   # the device buffer ``GalleryIndex.add_descriptors`` uploads host rows through
COMPACT_HOST_ROWS = 4096      # rows per piece (12 MB) of a host-side move whose destination meets its source


# The stored fields, one row per array, in the order ``save`` writes them (``row_off_host`` as ``row_off``; not the last).
# axis: what the first dimension counts, "rows" (keypoints), "edges", "entries" or "entries+1" (offsets); place: "device",
# "host", or "rows32" (the device, or pinned host memory in HOST_LAYOUTS); when: None (every index), the layouts that hold
# it, or "optional" (may be None).  Everything that enumerates the arrays loops over this table: a new field is a new row.
Field = namedtuple("Field", "name axis tail dtype place when")
_D = C.NODE_FEATURE_DIM
FIELDS = (
    Field("y", "rows", (_D,), torch.float32, "rows32", None),
    Field("row_off_host", "entries+1", (), torch.int64, "host", None),
    Field("n", "entries", (), torch.int32, "host", None),
    Field("src", "edges", (), torch.int32, "device", None),
    Field("dst", "edges", (), torch.int32, "device", None),
    Field("pseudo", "edges", (2,), torch.float32, "device", None),
    Field("edge_off", "entries+1", (), torch.int64, "host", None),
    Field("w", "entries", (C.GLOBAL_FEATURE_DIM,), torch.float32, "device", None),
    Field("P", "rows", (2,), torch.float32, "device", "optional"),
    Field("y16", "rows", (_D,), torch.bfloat16, "device", BF16_LAYOUTS),
    Field("subject", "entries", (), torch.int64, "host", "optional"),
    Field("y8", "rows", (_D,), torch.float8_e4m3fn, "device", (FP8_LAYOUT,)),
    Field("s8", "rows", (), torch.float32, "device", (FP8_LAYOUT,)),
    Field("desc", "entries", (_D,), torch.bfloat16, "device", "optional"),
    Field("row_off", "entries+1", (), torch.int64, "device", None),
)
FIELD = {f.name: f for f in FIELDS}
# the row stores of the layouts: what the enrolment loops write and ``ops.rows_move`` compacts
ROW_STORES = tuple(f for f in FIELDS if f.axis == "rows" and f.when != "optional")
# what the constructor says of a field that is not as its row of the table has it
_MUST = {"y16": "y16 must be bfloat16 of y's shape on the index device",
         "y8": "y8 must be float8_e4m3fn of y's shape and s8 float32, one scale per row, both on the index device",
         "desc": "desc must be bfloat16, one row of %d channels per entry, on the index device" % _D}
_MUST["s8"] = _MUST["y8"]


def _fields(layout, optional=()):
    """The rows of FIELDS an index of ``layout`` holds; of the optional ones those named in ``optional``."""
    return [f for f in FIELDS if f.when is None or (f.name in optional if f.when == "optional" else layout in f.when)]


def _count(axis, G, R, E):
    """The length of ``axis`` in an index (or a prefix) of G entries, R rows and E edges."""
    return {"rows": R, "edges": E, "entries": G, "entries+1": G + 1}[axis]


def _host_rows(shape, dev):
    """An uninitialised fp32 host tensor for an index on ``dev``: pinned when that is a GPU (the
    kernels read it through its device mapping), plain on a CPU "device"."""
    return torch.empty(shape, dtype=torch.float32, pin_memory=torch.device(dev).type == "cuda")


def _new_field(f, sizes, layout, dev):
    """Field ``f`` for ``sizes`` = (entries, rows, edges), allocated where it lives in an index of ``layout`` on
    ``dev``: the host tables and the offsets zero, everything else uninitialised."""
    shape = (_count(f.axis, *sizes),) + f.tail
    if f.place == "rows32" and layout in HOST_LAYOUTS:
        return _host_rows(shape, dev)
    make = torch.zeros if f.place == "host" or f.axis == "entries+1" else torch.empty
    return make(shape, dtype=f.dtype, device="cpu" if f.place == "host" else dev)


def _placed(f, t, layout, dev, at=None):
    """``t`` (``at``: its rows ``at``, an index where ``t`` is) where field ``f`` of an index of ``layout`` on ``dev``
    lives: a host table as it is, the fp32 rows of a host layout in host rows of their own, the rest on the device."""
    if f.place == "rows32" and layout in HOST_LAYOUTS:
        out = _host_rows((t.shape[0] if at is None else at.numel(),) + tuple(t.shape[1:]), dev)
        return out.copy_(t) if at is None else torch.index_select(t, 0, at, out=out)
    t = t if at is None else t[at]
    return t if f.place == "host" else t.to(dev)


def _make_store(cap, layout, dev, optional=()):
    """The buffers of an index with capacity ``cap`` = (entries, rows, edges): ``cap`` and every field by name, None
    for one the index does not hold (``_fields``).  The public fields of the index are prefix views of these."""
    have = _fields(layout, optional)
    return dict(cap=tuple(cap), **{f.name: _new_field(f, cap, layout, dev) if f in have else None for f in FIELDS})


def _fill(st, src, G, R, E):
    """``src(name)`` over the prefix of every field the storage ``st`` holds, but the device offsets (``_commit``'s)."""
    for f in FIELDS:
        if st[f.name] is not None and f.name != "row_off":
            st[f.name][:_count(f.axis, G, R, E)].copy_(src(f.name))


def _row_buffers(layout, get):
    """The row stores ``get(field)`` gives, by name; the fp32 rows as "y" on the device, "y_host" on the host."""
    b = {f.name: get(f) for f in ROW_STORES}
    b["y"], b["y_host"] = (None, b["y"]) if layout in HOST_LAYOUTS else (b["y"], None)
    return b


def _alloc_rows(layout, dev, rows):
    """The row buffers (``_row_buffers``) of a new index of exactly ``rows`` rows."""
    return _row_buffers(layout, lambda f: _new_field(f, (0, rows, 0), layout, dev) if f in _fields(layout) else None)


def _store_rows(index):
    """The same of an index with capacity: its storage, which the loops write past ``used``."""
    return _row_buffers(index.layout, lambda f: index._store[f.name])


def _check_capacity(what, capacity, G, R, E=0):
    """``capacity`` as given, (entries, keypoints[, edges]) -> (entries, rows, edges), each at least what is
    held already (G entries, R rows, E edges); ``edges`` defaults to 6 per row."""
    try:
        cap = [int(v) for v in capacity]
    except TypeError:
        cap = []
    if len(cap) not in (2, 3):
        raise FpmError("%s: capacity must be (entries, keypoints) or (entries, keypoints, edges)" % what)
    if len(cap) == 2:
        cap.append(6 * cap[1])
    if cap[0] < max(G, 1) or cap[1] < max(R, 1) or cap[2] < max(E, 1):
        raise FpmError("%s: capacity %s below the %d entries, %d rows and %d edges to hold" % (what, tuple(cap), G, R, E))
    if cap[0] > 2 ** 31 - 2:
        raise FpmError("%s: entry numbers must fit int32" % what)
    return tuple(cap)


def _edge_room(what, seen, room):
    """Refuse an enrolment into an index whose edges (``seen`` so far) pass the ``room`` left (None: no bound)."""
    if room is not None and seen > room:
        raise FpmError("%s: the graphs' edges pass the index's capacity (%d so far, room for %d); reserve a bigger "
                       "index (GalleryIndex.reserve(..., edges=...))" % (what, seen, room))


def _entry_ranges(off, ent):
    """The numbers off[e] .. off[e + 1] of every entry e of ``ent``, concatenated -> (host int64 index, the
    entries' new offsets)."""
    cnt = off[ent + 1] - off[ent]
    new = torch.cat([torch.zeros(1, dtype=torch.int64), cnt.cumsum(0)])
    at = torch.arange(int(new[-1]), dtype=torch.int64)
    return at + torch.repeat_interleave(off[ent] - new[:-1], cnt), new


def _check_subjects(what, labels, G):
    """Subject labels as given -> host int64 (G,), a copy: one integer >= 0 per entry."""
    t = torch.as_tensor(labels)
    if t.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
        raise FpmError("%s: subject labels must be integers (got %s)" % (what, t.dtype))
    if t.dim() != 1 or int(t.numel()) != int(G):
        raise FpmError("%s: %s subject labels for %d entries (one label per entry)" % (what, tuple(t.shape), G))
    t = t.detach().cpu().to(torch.int64).clone()
    if int(G) and int(t.min()) < 0:
        raise FpmError("%s: a negative subject label (%d)" % (what, int(t.min())))
    return t


def _select_host(index, select, what):
    """The entries a query runs over (host int64): ``select`` as given, or all entries: the live ones of an
    index with removed slots (the one place that defines "all entries"); a removed entry is refused."""
    if select is None:
        return index.live
    sel = torch.as_tensor(select, dtype=torch.int64).view(-1).cpu()
    if sel.numel() == 0 or int(sel.min()) < 0 or int(sel.max()) >= index.G:
        raise FpmError("%s: select must name entries in [0, %d)" % (what, index.G))
    index._check_live(sel, what)
    return sel


class GalleryIndex:
    """Data of an enrolled gallery of G graphs (a container; ``Net.enroll`` fills it):

      y         (sum n, 768) fp32   SplineConv output rows, graph g at [row_off[g], row_off[g + 1]);
                                    on the device, or ("bf16+host", "fp8+host") in pinned host memory
      y16       (sum n, 768) bf16   device; the same rows rounded to nearest even (``ops.cast_bf16``),
                                    what the coarse kernels read; None in the "f32" and "fp8+host" layouts
      y8, s8    (sum n, 768) e4m3,  device, "fp8+host" only (else None): the rows quantised with one power-of-two
                (sum n,) fp32       scale per row (``ops.rows_quant8``); the coarse operand is bf16(y8 * s8)
      layout    "f32"               y on the device (3 KB per keypoint), no y16
                "f32+bf16"          y and y16 on the device (4.5 KB per keypoint)
                "bf16+host"         y16 on the device (1.5 KB per keypoint), y on the host: the coarse
                                    pass reads y16, the exact forward ``fetch``es the rows it needs
                "fp8+host"          y8 and s8 on the device (772 B per keypoint), y on the host: the coarse
                                    pass reads y8 and s8, the exact forward ``fetch``es as above
      row_off   (G + 1,) int64      device (the index's device, whatever the layout); ``row_off_host``
                                    its host copy
      n         (G,) int32          keypoints per graph (host)
      src, dst  (sum E,) int32      each graph's edges, graph-local node ids, concatenated (device)
      pseudo    (sum E, 2) fp32     their pseudo-coordinates (device)
      edge_off  (G + 1,) int64      edge offsets per graph (host)
      w         (G, 512) fp32       global features (device)
      desc      (G, 768) bf16       device, or None: the prescreen descriptor of each entry, its rows sum-pooled
                                    and L2-normalised (``ops.rows_pool``; ``add_descriptors``,
                                    ``enroll*(descriptors=True)``): 1536 B per entry
      P         (sum n, 2) fp32     keypoints, or None when the graphs carry none (device)
      subject   (G,) int64 or None  the subject label (>= 0) of each entry (host; ``set_subjects``): the
                                    impressions of one finger share a label.  ``subject_groups`` makes a
                                    selection's CSR group tables, which ``identify(by="subject")`` fuses by
      sc_mode   "f32" | "bf16"      the SplineConv arithmetic that produced y
      _pack_gen, weights_id         the enrolling net's weight-pack generation and a digest of its
                                    SplineConv weights (``Net.identify`` refuses other weights)
    """

    def __init__(self, y, row_off, n, src, dst, pseudo, edge_off, w, P, sc_mode, pack_gen, weights_id, y16=None,
                 layout="f32", subject=None, y8=None, s8=None, desc=None):
        self._init_state(sc_mode, pack_gen, weights_id, layout)
        given = dict(y=y, y16=y16, y8=y8, s8=s8, P=P, src=src, dst=dst, pseudo=pseudo, w=w, desc=desc, row_off=row_off)
        for when in dict.fromkeys(f.when for f in FIELDS if isinstance(f.when, tuple)):
            names = [f.name for f in FIELDS if f.when == when]
            has = [given[k] is not None for k in names]
            if not all(has) if layout in when else any(has):
                raise FpmError("GalleryIndex: layout %r %s" % (layout, "needs " + " and ".join(names) if layout in when
                                                               else "has no " + " and no ".join(names)))
        sizes = (int(w.shape[0]), int(y.shape[0]), int(src.numel()))
        for k, t in given.items():
            if k in _MUST and t is not None and (
                    not isinstance(t, torch.Tensor) or t.dtype != FIELD[k].dtype or t.device != row_off.device
                    or tuple(t.shape) != (_count(FIELD[k].axis, *sizes),) + FIELD[k].tail):
                raise FpmError("GalleryIndex: inconsistent fields (%s)" % _MUST[k])
        if layout in HOST_LAYOUTS and (y.is_cuda or (row_off.is_cuda and not y.is_pinned())):
            raise FpmError("GalleryIndex: layout %r keeps y in host memory (pinned when the index is on a GPU)" % layout)
        vars(self).update(given)
        self.row_off_host = row_off.cpu()
        self.n = torch.as_tensor(n, dtype=torch.int32).cpu()
        self.edge_off = torch.as_tensor(edge_off, dtype=torch.int64).cpu()
        self.subject = None         # (G,) int64 host subject labels (set_subjects), or None
        self._check_tables()
        if subject is not None:
            self.set_subjects(subject)

    def _init_state(self, sc_mode, pack_gen, weights_id, layout):
        """Everything of a new index but its arrays."""
        if sc_mode not in ("f32", "bf16"):
            raise FpmError("GalleryIndex: sc_mode must be 'f32' or 'bf16'")
        if layout not in LAYOUTS:
            raise FpmError("GalleryIndex: layout must be one of %s" % (LAYOUTS,))
        self.layout, self.sc_mode = layout, sc_mode
        self._pack_gen = int(pack_gen)
        self.weights_id = str(weights_id)
        self._stage = None          # fetch: (sel, staging buffer, row offsets device / host) of the last selection
        self._sel = None            # the last selection's side-1 batch data (_selection)
        self._groups = None         # the last selection's group tables (subject_groups)
        self._store = None          # the buffers at capacity the fields are prefix views of (reserve), or None
        self._removed = None        # host bool table over the slots (remove); None: nothing was ever removed
        self._live = None           # the live slots, while the table above is unchanged
        self.generation = 0         # bumped by every mutation (enroll_into, remove, compact)
        self.last_compact = None    # the last compaction's launches by route (compact)

    def _check_tables(self):
        """The offsets, counts and sizes of the arrays agree (and no label of a storage's table is negative)."""
        G = self.G
        if (self.row_off.dtype != torch.int64 or self.row_off_host.numel() != G + 1 or self.edge_off.numel() != G + 1
                or int(self.row_off_host[-1]) != self.y.shape[0] or int(self.edge_off[-1]) != self.src.numel()
                or not torch.equal(self.row_off_host[1:] - self.row_off_host[:-1], self.n.long())
                or tuple(self.w.shape) != (G, C.GLOBAL_FEATURE_DIM) or self.y.dtype != torch.float32
                or (self.subject is not None and G and int(self.subject.min()) < 0)):
            raise FpmError("GalleryIndex: inconsistent fields")

    @property
    def G(self):
        return int(self.n.numel())

    @property
    def device(self):
        return self.row_off.device

    def _bytes(self, on_host):
        """The bytes of the arrays (the storage's, if any) on the device, or of those a host layout keeps on the host."""
        at = self._store or vars(self)
        ts = [at[f.name] for f in FIELDS
              if f.place != "host" and (f.place == "rows32" and self.layout in HOST_LAYOUTS) == on_host]
        return sum(t.numel() * t.element_size() for t in ts if t is not None)

    def nbytes(self):
        """Device bytes held: the rows (3 KB per keypoint in the "f32" layout, 4.5 KB in "f32+bf16",
        1.5 KB in "bf16+host", 772 B in "fp8+host"), plus edges, global features and the descriptors (1536 B per
        entry) when the index holds them."""
        groups = [] if self._groups is None else [self._groups[1][k] for k in ("labels_d", "off_d", "pos_d")]
        return self._bytes(False) + sum(t.numel() * t.element_size() for t in groups)

    def host_nbytes(self):
        """Host bytes held: the fp32 rows of the "bf16+host" and "fp8+host" layouts (3 KB per keypoint), else 0."""
        return self._bytes(True)

    def coarse_rows(self):
        """What the coarse kernels read -> (rows, row_scale): the bf16 copy when the index keeps one, the e4m3
        rows and their scales in "fp8+host", else the fp32 rows (``ops.coarse_score(rows, ..., row_scale=)``)."""
        if self.y8 is not None:
            return self.y8, self.s8
        return (self.y if self.y16 is None else self.y16), None

    def add_descriptors(self, chunk=None):
        """Pool the prescreen descriptor of every slot of an existing index (``ops.rows_pool``) -> self, with
        ``desc`` (G, 768) bf16 on the device (in an index with capacity: a table of ``capacity`` entries, of which
        ``desc`` is the prefix view).  The "f32" layouts pool from ``y`` where it is; "bf16+host" and "fp8+host"
        upload their pinned fp32 rows in chunks of whole entries of at most ``chunk`` rows (default
        DESC_STAGE_BYTES worth, never less than the largest entry) into one reused device buffer.  The bits are
        those ``enroll*(descriptors=True)`` gives.  Removed slots are pooled too (their rows are still there);
        an index that holds descriptors already pools them afresh."""
        G, R, _ = self.used
        dev = self.device
        with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
            desc = (_new_field(FIELD["desc"], self.used, self.layout, dev) if self._store is None
                    else self._gain("desc")[:G])
            ro = self.row_off_host
            if self.layout not in HOST_LAYOUTS:
                ops.rows_pool(self.y, self.row_off, 0, G, out=desc, row_off_host=ro)
            elif G:
                big = int(self.n.max())
                rows = max(DESC_STAGE_BYTES // ROW_BYTES if chunk is None else int(chunk), 1)
                if rows < big:
                    if chunk is not None:
                        raise FpmError("GalleryIndex.add_descriptors: chunk = %d below the largest entry (%d rows)"
                                       % (rows, big))
                    rows = big
                stage = torch.empty(min(rows, R), C.NODE_FEATURE_DIM, device=dev, dtype=torch.float32)
                g0 = 0
                while g0 < G:
                    # the entries [g0, g1) whose rows fit the stage: at least one
                    g1 = int(torch.searchsorted(ro, ro[g0] + rows, right=True)) - 1
                    g1 = min(max(g1, g0 + 1), G)
                    r0, r1 = int(ro[g0]), int(ro[g1])
                    stage[:r1 - r0].copy_(self.y[r0:r1], non_blocking=True)
                    off = ro[g0:g1 + 1] - r0
                    ops.rows_pool(stage[:r1 - r0], off.to(dev), 0, g1 - g0, out=desc[g0:g1], row_off_host=off)
                    g0 = g1
        self.desc = desc
        return self

    # ---- a mutable index: capacity, enrolment into it (Net.enroll_into), tombstones, compaction ----
    @property
    def used(self):
        """(entries, rows, edges) the index holds; removed slots count until ``compact``."""
        return self.G, int(self.y.shape[0]), int(self.src.numel())

    @property
    def capacity(self):
        """(entries, rows, edges) the storage is sized for (``reserve``, ``enroll*(capacity=...)``), or None:
        an index that holds exactly what it was enrolled with.  ``compact`` on such an index makes its own
        tensors its storage: afterwards ``capacity`` is what the index held before, and the room the removed
        entries left can be enrolled into."""
        return None if self._store is None else self._store["cap"]

    @property
    def removed(self):
        """(G,) host bool: the slots ``remove`` marked dead."""
        if self._removed is None:
            return torch.zeros(self.G, dtype=torch.bool)
        return self._removed[:self.G]

    @property
    def tombstones(self):
        """Whether some slot is marked dead."""
        return self._removed is not None and int(self.live.numel()) != self.G

    @property
    def live(self):
        """The live slots, ascending (host int64): what a query with ``select=None`` searches."""
        if self._removed is None:
            return torch.arange(self.G, dtype=torch.int64)
        if self._live is None:
            self._live = torch.nonzero(~self._removed[:self.G]).view(-1)
        return self._live

    def _check_live(self, sel, what):
        """Refuse entry numbers ``sel`` (host int64, in range) that name a removed slot."""
        if self.tombstones and bool(self._removed[sel].any()):
            raise FpmError("%s: entry %d was removed from the index" % (what, int(sel[self._removed[sel]][0])))

    def _touch(self):
        """What every mutation ends with: the caches of the last selection go (the staging buffer of
        ``fetch`` stays, without its key) and ``generation`` is bumped."""
        self._sel = self._groups = self._live = None
        if self._stage is not None:
            self._stage = (torch.empty(0, dtype=torch.int64), self._stage[1], None, None, None)
        self.generation += 1

    def _commit(self, G, R, E, lo=0):
        """The one writer of the public fields of an index with storage: they become the prefix views of
        the storage for ``G`` entries, ``R`` rows and ``E`` edges, the device offsets of the slots from
        ``lo`` on are uploaded from the host table, and the caches are dropped (``_touch``)."""
        st = self._store
        st["row_off"][lo:G + 1].copy_(st["row_off_host"][lo:G + 1])
        for f in FIELDS:
            t = st[f.name]
            setattr(self, f.name, None if t is None else t[:_count(f.axis, G, R, E)])
        self._touch()

    @staticmethod
    def _over(st, G, R, E, sc_mode, pack_gen, weights_id, layout):
        """The index over the first G entries, R rows and E edges of the storage ``st``, its tables checked."""
        idx = object.__new__(GalleryIndex)
        idx._init_state(sc_mode, pack_gen, weights_id, layout)
        idx._store = st
        idx._commit(G, R, E)
        idx._check_tables()
        idx.generation = 0
        return idx

    def _gain(self, name):
        """The storage's optional field ``name``, allocated at capacity if the storage does not hold it yet."""
        st = self._store
        if st[name] is None:
            st[name] = _new_field(FIELD[name], st["cap"], self.layout, self.device)
        return st[name]

    def reserve(self, entries, keypoints, edges=None):
        """A new index holding this index's entries (and tombstones) in storage sized for ``entries`` slots,
        ``keypoints`` rows and ``edges`` edges (default 6 per row: a planar triangulation has at most 6n - 12
        directed edges, which covers ``stg="tri"`` graphs; host-dict graphs with more pass ``edges``), so
        that ``Net.enroll_into`` can add entries without enrolling the gallery again.  In the "bf16+host"
        and "fp8+host" layouts the pinned host rows are allocated here, once, at capacity.  This index is untouched; to
        grow a full index, reserve a bigger one: nothing is ever re-allocated under a live index."""
        G, R, E = self.used
        cap = _check_capacity("GalleryIndex.reserve", (entries, keypoints) if edges is None else
                              (entries, keypoints, edges), G, R, E)
        dev = self.device
        with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
            st = _make_store(cap, self.layout, dev, [k for k in FIELD if getattr(self, k) is not None])
            _fill(st, lambda k: getattr(self, k), G, R, E)
            idx = GalleryIndex._over(st, G, R, E, self.sc_mode, self._pack_gen, self.weights_id, self.layout)
        if self._removed is not None:
            idx._removed = torch.zeros(cap[0], dtype=torch.bool)
            idx._removed[:G] = self._removed[:G]
        return idx

    def _adopt(self):
        """The storage of an index that has none: its own tensors, full (capacity = used)."""
        if self._store is None:
            self._store = dict(cap=self.used, **{f.name: getattr(self, f.name) for f in FIELDS})
        return self._store

    def _need_capacity(self, what):
        if self._store is None:
            raise FpmError("%s: the index has no capacity; make one with GalleryIndex.reserve(entries, keypoints) "
                           "or enroll*(capacity=...)" % what)

    def _begin_append(self, what, Gn, Rn, subjects, has_P):
        """The refusals of an append of ``Gn`` entries of ``Rn`` rows, before anything is written -> (G, R, E)
        now: the slot, row and edge where the new entries' data goes, past ``used``."""
        self._need_capacity(what)
        if (subjects is None) != (self.subject is None):
            raise FpmError("%s: the index %s, the call %s" % (
                what, "has subject labels" if subjects is None else "has no subject labels",
                "gives none (subjects=...)" if subjects is None else "gives subjects"))
        if has_P != (self.P is not None):
            raise FpmError("%s: the index %s keypoints P, the new graphs %s" % (
                what, "keeps" if not has_P else "keeps no", "carry none" if not has_P else "carry them"))
        G, R, E = self.used
        cap = self._store["cap"]
        if G + Gn > cap[0] or R + Rn > cap[1]:
            raise FpmError("%s: %d entries and %d rows more pass the index's capacity (%d of %d entries, %d of %d rows "
                           "used); reserve a bigger index (GalleryIndex.reserve)" % (what, Gn, Rn, G, cap[0], R, cap[1]))
        return G, R, E

    def _finish_append(self, what, at, n, w, P, src, dst, pseudo, cnt, subjects, desc=None):
        """The end of an append whose rows are written (past ``used``, from ``at`` = ``_begin_append``'s):
        the new entries' small arrays go into the storage's tail -- n host int32, w (Gn, 512), P (Rn, 2) or
        None, the edges with graph-local ids and their host counts per entry, ``desc`` (Gn, 768) the new entries'
        descriptors on an index that holds them -- and the index is committed.
        Until the commit no field has changed: an error before it leaves the index as it was."""
        G, R, E = at
        st = self._store
        n = torch.as_tensor(n, dtype=torch.int32).view(-1).cpu()
        cnt = torch.as_tensor(cnt, dtype=torch.int64).view(-1).cpu()
        Gn, Rn, En = int(n.numel()), int(n.sum()), int(src.numel())
        if int(cnt.numel()) != Gn or int(cnt.sum()) != En:
            raise FpmError("%s: %d edges, their counts per entry sum to %d" % (what, En, int(cnt.sum())))
        _edge_room(what, En, st["cap"][2] - E)
        if (desc is None) != (st["desc"] is None):
            raise FpmError("%s: the index %s descriptors, the append %s" % (
                what, "holds" if desc is None else "holds no", "brings none" if desc is None else "brings them"))
        new = dict(w=w, desc=desc, P=P, src=src, dst=dst, pseudo=pseudo, n=n, row_off_host=R + n.long().cumsum(0),
                   edge_off=E + cnt.cumsum(0), subject=subjects)
        for k, t in new.items():        # each into the tail of its field: from its axis' used count to the new one
            if k == "n" and self.layout in HOST_LAYOUTS and self.device.type == "cuda":
                torch.cuda.current_stream(self.device).synchronize()   # the host rows are complete before they are read
            if t is not None:
                st[k][_count(FIELD[k].axis, G, R, E):_count(FIELD[k].axis, G + Gn, R + Rn, E + En)].copy_(t)
        self._commit(G + Gn, R + Rn, E + En, lo=G)
        return torch.arange(G, G + Gn, dtype=torch.int64)

    def remove(self, entries):
        """Mark the entries ``entries`` dead (tombstones in the host table ``removed``).  Entry numbers stay
        as they are and ``G`` still counts slots; no row is touched.  Every query then searches ``live``:
        ``select=None`` means the live entries, and a ``select``, ``probe_select``, pair, ``slice`` or
        ``fetch`` that names a removed slot is refused.  ``compact`` squeezes the dead slots out.  Refused:
        an entry outside [0, G), named twice or removed already, and removing the last live entry."""
        ent = torch.as_tensor(entries, dtype=torch.int64).view(-1).cpu()
        if ent.numel() == 0 or int(ent.min()) < 0 or int(ent.max()) >= self.G:
            raise FpmError("GalleryIndex.remove: entries must name entries in [0, %d)" % self.G)
        if int(torch.unique(ent).numel()) != int(ent.numel()):
            raise FpmError("GalleryIndex.remove: an entry is named twice")
        if bool(self.removed[ent].any()):
            raise FpmError("GalleryIndex.remove: entry %d was removed already" % int(ent[self.removed[ent]][0]))
        if int(ent.numel()) >= int(self.live.numel()):
            raise FpmError("GalleryIndex.remove: this would remove the last live entry of the index")
        if self._removed is None:
            self._removed = torch.zeros(self.G if self._store is None else self._store["cap"][0], dtype=torch.bool)
        self._removed[ent] = True
        self._touch()

    def compact(self, stage_rows=None):
        """Squeeze the removed slots out, inside the same storage -> ``new_of_old`` (G_old,) host int64: the
        new number of every old entry, -1 for a removed one.  Afterwards every field equals
        ``slice(live)`` of the index before; capacity is unchanged and nothing is allocated but the stage.
        An index without capacity keeps its own tensors as its storage from here on (``capacity``: what it
        held before; the freed room can be enrolled into; ``slice(live)`` instead makes a tight copy).

        Unlike an append, a compaction is not atomic: rows are overwritten as it goes and the tables change
        at the end, so an error midway (none is expected once the first launch is out: every refusal and
        the one allocation, the stage, come before it) would leave rows that the tables no longer describe.

        The rows (97 % of the bytes) move by ``ops.rows_move``, in blocks of consecutive live entries of at
        most ``stage_rows`` rows (default COMPACT_STAGE_BYTES worth, never less than the largest entry; a
        given value below the largest moved entry is refused).  Live entries only move towards the front
        and blocks ascend, so a block's destination covers only rows that are dead or were read already.  A
        block whose destination ends at or before its source begins moves in one launch, storage to
        storage; any other block in two on one stream, storage to stage, stage to storage (the stage: one
        device buffer reused by every such block).  No launch reads rows that it writes; ``ops.rows_move``
        checks that on the host each time.  ``last_compact`` counts the blocks by route.  The small arrays
        (P, edges, w, offsets, the host tables; 3 % of the bytes) are gathered out of place with torch
        indexing and copied back over the prefix.  In "fp8+host" the e4m3 rows and their scales move as the
        bf16 rows do (``ops.rows_move(src8=...)``).  The host fp32 rows of "bf16+host" / "fp8+host" are moved by host
        code after a device synchronise (kernels read that memory through its mapping): ascending, one
        copy per run of adjacent live entries, a run that lands on rows it still occupies in pieces of
        COMPACT_HOST_ROWS rows through a temporary."""
        G, R, E = self.used
        live = self.live
        L = int(live.numel())
        new_of_old = torch.full((G,), -1, dtype=torch.int64)
        new_of_old[live] = torch.arange(L, dtype=torch.int64)
        self.last_compact = dict(direct=0, staged=0, launches=0, rows=0)
        if L == G:
            return new_of_old
        ro, eo = self.row_off_host, self.edge_off
        cnt, src = ro[live + 1] - ro[live], ro[live]
        new_ro = torch.cat([torch.zeros(1, dtype=torch.int64), cnt.cumsum(0)])
        dst = new_ro[:-1]
        first = int(torch.nonzero(live != torch.arange(L)).view(-1)[0]) if L and int(live[-1]) != L - 1 else L
        big = int(cnt[first:].max()) if first < L else 0
        if stage_rows is None:
            stage_rows = max(COMPACT_STAGE_BYTES // ROW_BYTES, big)
        stage_rows = int(stage_rows)
        if stage_rows < max(big, 1):
            raise FpmError("GalleryIndex.compact: stage_rows = %d below the largest entry to move (%d rows)"
                           % (stage_rows, big))
        # blocks [a, b) of the moved live entries: at most stage_rows rows and 65535 segments each
        blocks, a, rows = [], first, 0
        for i in range(first, L):
            k = int(cnt[i])
            if i > a and (rows + k > stage_rows or i - a >= 65535):
                blocks.append((a, i))
                a, rows = i, 0
            rows += k
        if a < L:
            blocks.append((a, L))
        st = self._adopt()
        dev = self.device
        host_rows = self.layout in HOST_LAYOUTS
        y32, y16, y8, s8 = None if host_rows else st["y"], st["y16"], st["y8"], st["s8"]
        if y8 is not None:
            # the fp8 layout's one row store on the device; (source, destination) -> the keywords of ops.rows_move
            rows_kw = lambda s, d: dict(src8=y8 if s else g8, dst8=y8 if d else g8, srcs=s8 if s else gs,
                                        dsts=s8 if d else gs)
        else:
            rows_kw = lambda s, d: dict(src32=y32 if s else s32, dst32=y32 if d else s32, src16=y16 if s else s16,
                                        dst16=y16 if d else s16)
        with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
            if blocks:
                stg = torch.cat([dst[a:b] - dst[a] for a, b in blocks])          # offsets into the stage
                src_h, dst_h, cnt_h = src[first:].contiguous(), dst[first:].contiguous(), cnt[first:].contiguous()
                src_d, dst_d, cnt_d, stg_d = src_h.to(dev), dst_h.to(dev), cnt_h.to(dev), stg.to(dev)
            # the stage, before the first launch: once rows have moved nothing may fail
            s32 = s16 = g8 = gs = None
            if any(int(new_ro[b]) > int(src[a]) for a, b in blocks):
                if y8 is not None:
                    g8 = torch.empty(stage_rows, C.NODE_FEATURE_DIM, device=dev, dtype=torch.float8_e4m3fn)
                    gs = torch.empty(stage_rows, device=dev, dtype=torch.float32)
                if y32 is not None:
                    s32 = torch.empty(stage_rows, C.NODE_FEATURE_DIM, device=dev, dtype=torch.float32)
                if y16 is not None:
                    s16 = torch.empty(stage_rows, C.NODE_FEATURE_DIM, device=dev, dtype=torch.bfloat16)
            for a, b in blocks:
                u, v = a - first, b - first
                host = dict(cnt_host=cnt_h[u:v])
                tabs = (src_d[u:v], dst_d[u:v], stg_d[u:v], src_h[u:v], dst_h[u:v], stg[u:v])
                self.last_compact["rows"] += int(cnt_h[u:v].sum())
                if int(new_ro[b]) <= int(src[a]):
                    ops.rows_move(tabs[0], tabs[1], cnt_d[u:v], src_off_host=tabs[3], dst_off_host=tabs[4], **host,
                                  **rows_kw(True, True))
                    self.last_compact["direct"] += 1
                    self.last_compact["launches"] += 1
                    continue
                ops.rows_move(tabs[0], tabs[2], cnt_d[u:v], src_off_host=tabs[3], dst_off_host=tabs[5], **host,
                              **rows_kw(True, False))
                ops.rows_move(tabs[2], tabs[1], cnt_d[u:v], src_off_host=tabs[5], dst_off_host=tabs[4], **host,
                              **rows_kw(False, True))
                self.last_compact["staged"] += 1
                self.last_compact["launches"] += 2
            if host_rows:
                if dev.type == "cuda":
                    torch.cuda.synchronize(dev)              # no kernel still reads the host rows through the mapping
                y = st["y"]
                # runs of adjacent live entries: each is one range of rows before and after
                head = torch.ones(L - first, dtype=torch.bool)
                head[1:] = src[first + 1:] != src[first:-1] + cnt[first:-1]
                at = (torch.nonzero(head).view(-1) + first).tolist() + [L]
                for i, j in zip(at[:-1], at[1:]):
                    s, d, k = int(src[i]), int(dst[i]), int(new_ro[j] - new_ro[i])
                    step = max(s - d, COMPACT_HOST_ROWS)          # a piece no longer than the shift lands on rows already read
                    for o in range(0, k, step):
                        part = y[s + o:s + min(k, o + step)]
                        y[d + o:d + min(k, o + step)].copy_(part.clone() if step > s - d else part)
            # the small arrays: gathered out of place by their axis (the right sides are whole before anything is written)
            rows_at, _ = _entry_ranges(ro, live)
            edges_at, new_eo = _entry_ranges(eo, live)
            Rn, En = int(new_ro[-1]), int(new_eo[-1])
            at = dict(rows=rows_at, edges=edges_at, entries=live)
            at_d = {k: v.to(dev) for k, v in at.items()}
            for f in FIELDS:
                if f.axis in at and f not in ROW_STORES and st[f.name] is not None:
                    pick = (at if f.place == "host" else at_d)[f.axis]
                    st[f.name][:pick.numel()] = st[f.name][pick]
            st["row_off_host"][:L + 1], st["edge_off"][:L + 1] = new_ro, new_eo
            self._removed[:] = False
            self._commit(L, Rn, En)
        return new_of_old

    def save(self, path):
        """``torch.save`` of a dict of tensors and scalars (no pickled code objects).  An "f32" index
        writes format 1, as ever; the bf16 layouts write format 2, with ``layout`` and ``y16``.  Of an
        index with capacity the used part is written; one with removed slots writes format 3, which adds
        the table ``removed``.  "fp8+host" writes format 4: ``layout``, ``y8`` (as bytes: uint8) and ``s8`` in
        ``y16``'s place, and ``removed`` when there are removed slots.  An index that holds descriptors writes
        format 5: ``layout``, the layout's own row fields as above, ``desc``, and ``removed`` when there are removed
        slots; without descriptors the formats 1 to 4 are written as before."""
        # a field of an index with storage is a view: a host view is copied, so that only its part is written
        host = (lambda t: t.cpu()) if self._store is None else (lambda t: t.cpu() if t.is_cuda else t.clone())
        fmt = (FORMAT_DESC if self.desc is not None else FORMAT_FP8 if self.layout == FP8_LAYOUT else
               FORMAT_TOMBSTONES if self.tombstones else FORMAT_LAYOUTS if self.layout in BF16_LAYOUTS else FORMAT)
        d = dict(format=fmt)
        for f in FIELDS:                    # in file order, with the scalars, ``layout`` and ``removed`` at their places
            t = getattr(self, f.name)
            if f.name == "y16" and t is not None:
                d["layout"] = self.layout   # where format 2 put it; the later formats after ``subject``
            if t is not None and f.name != "row_off":
                t = host(t)
                d["row_off" if f.name == "row_off_host" else f.name] = t.view(torch.uint8) if t.element_size() == 1 else t
            if f.name == "w":
                d.update(sc_mode=self.sc_mode, pack_gen=self._pack_gen, weights_id=self.weights_id)
            if f.name == "subject" and fmt != FORMAT:
                d.setdefault("layout", self.layout)
            if f.name == "subject" and self.tombstones:
                d["removed"] = self.removed.clone()
        torch.save(d, path)

    @staticmethod
    def load(path, device, capacity=None):
        """The index ``save`` wrote, on ``device``.  ``capacity``: (entries, keypoints[, edges]) -- the index
        is restored into storage of that size (as ``reserve`` makes it), without a second copy of it."""
        d = torch.load(path, map_location="cpu", weights_only=True)
        fmt, named = d.get("format"), d.get("layout")
        layout = "f32" if fmt == FORMAT else named
        # the fp8 layout came with format 4, which is that layout's alone; format 5 is every layout's, and alone has desc
        if not (fmt in FORMATS and layout in LAYOUTS and ((named == FP8_LAYOUT) == (fmt == FORMAT_FP8) or fmt == FORMAT_DESC)
                and ("desc" in d) == (fmt == FORMAT_DESC) and ("removed" in d or fmt != FORMAT_TOMBSTONES)
                and all(f.name in d for f in FIELDS if isinstance(f.when, tuple) and layout in f.when)):
            raise FpmError("GalleryIndex.load: %s is not a gallery index of format %d, %d, %d, %d or %d"
                           % ((path,) + FORMATS))
        if layout == FP8_LAYOUT:
            d["y8"] = d["y8"].view(torch.float8_e4m3fn)
        scalars = dict(sc_mode=d["sc_mode"], pack_gen=d["pack_gen"], weights_id=d["weights_id"], layout=layout)
        if capacity is None:
            fields = {f.name: _placed(f, d[f.name], layout, device)
                      for f in _fields(layout, set(d)) if f.name != "row_off_host"}
            fields.setdefault("P", None)                 # the one optional field the constructor has no default for
            idx = GalleryIndex(**scalars, **fields)
        else:
            G, R, E = int(d["n"].numel()), int(d["y"].shape[0]), int(d["src"].numel())
            cap = _check_capacity("GalleryIndex.load", capacity, G, R, E)
            dev = torch.device(device)
            with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
                st = _make_store(cap, layout, dev, set(d))
                _fill(st, lambda k: d["row_off" if k == "row_off_host" else k], G, R, E)
                idx = GalleryIndex._over(st, G, R, E, **scalars)
        if "removed" in d:
            idx._removed = torch.zeros(idx.G if capacity is None else idx.capacity[0], dtype=torch.bool)
            idx._removed[:idx.G] = d["removed"]
        return idx

    def set_subjects(self, labels):
        """Label (or relabel) the entries: ``labels`` (G,) integers >= 0, the subject of each entry (the
        impressions of one finger share a label; removed slots are labelled too).  Kept as a host int64
        tensor (``subject``); the cached group tables are dropped.  None removes the labels."""
        lab = None if labels is None else _check_subjects("set_subjects", labels, self.G)
        if self._store is not None:
            if lab is None:
                self._store["subject"] = None
            else:
                self._gain("subject")[:self.G] = lab
                lab = self._store["subject"][:self.G]
        self.subject = lab
        self._groups = None

    def subject_groups(self, select=None):
        """The group tables of the entries ``select`` (None: all) by subject -> dict:
          labels  (S,) int64 host     the distinct labels of the selection, ascending (``labels_d``: device)
          off     (S + 1,) int32 host group s is pos[off[s]:off[s + 1]]          (``off_d``: device)
          pos     (Gs,) int32 host    positions into the selection, ascending inside a group (``pos_d``)
          group   (Gs,) int64 host    the group number of each position of the selection
        Built on the host with a stable sort of the selection's labels; independent of the probe, so the
        last selection's tables are kept for the next query (as ``_selection`` keeps its batch data)."""
        if self.subject is None:
            raise FpmError("subject_groups: the index has no subject labels (set_subjects, or enroll(subjects=...))")
        sel = _select_host(self, select, "subject_groups")
        if self._groups is not None and torch.equal(self._groups[0], sel):
            return self._groups[1]
        lab = self.subject[sel]
        order = torch.argsort(lab, stable=True)
        labels, cnt = torch.unique_consecutive(lab[order], return_counts=True)
        off = torch.cat([torch.zeros(1, dtype=torch.int64), cnt.cumsum(0)]).to(torch.int32)
        pos = order.to(torch.int32)
        group = torch.empty_like(order)
        group[order] = torch.repeat_interleave(torch.arange(int(labels.numel())), cnt)
        dev = self.device
        t = dict(labels=labels, off=off, pos=pos, group=group, labels_d=labels.to(dev), off_d=off.to(dev),
                 pos_d=pos.to(dev))
        self._groups = (sel, t)
        return t

    def fetch(self, sel):
        """The fp32 rows of the entries ``sel`` (host int64, in that order) of a "bf16+host" or "fp8+host" index, copied
        from the host into a device staging buffer (``ops.rows_fetch``: one kernel reads the pinned
        rows) -> (y_stage (sum of the selected n, 768) fp32 device, its row offsets (len(sel) + 1,)
        int64 on the device, the same on the host): entry sel[m] at rows [off[m], off[m + 1]).  The
        buffer is reused from call to call and grows as needed; a repeated selection is not copied
        again.  Selections over FETCH_MAX_BYTES of rows are refused."""
        if self.layout not in HOST_LAYOUTS:
            raise FpmError("GalleryIndex.fetch: layout %r holds its fp32 rows on the device" % self.layout)
        sel = torch.as_tensor(sel, dtype=torch.int64).view(-1).cpu()
        if sel.numel() == 0 or int(sel.min()) < 0 or int(sel.max()) >= self.G:
            raise FpmError("GalleryIndex.fetch: sel must name entries in [0, %d)" % self.G)
        self._check_live(sel, "GalleryIndex.fetch")
        if self._stage is not None and torch.equal(self._stage[0], sel):
            return self._stage[2:]
        ng = self.n[sel].long()
        total = int(ng.sum())
        if total * ROW_BYTES > FETCH_MAX_BYTES:
            raise FpmError("identify: the %d selected entries' fp32 rows take %d bytes on the device, over "
                           "FETCH_MAX_BYTES = %d; an index with its rows on the host (layout 'bf16+host' or 'fp8+host') runs "
                           "the exact forward over a shortlist: pass shortlist=M, or a smaller select"
                           % (sel.numel(), total * ROW_BYTES, FETCH_MAX_BYTES))
        dev = self.device
        buf = None if self._stage is None else self._stage[1]
        self._stage = None
        if buf is None or buf.shape[0] < total:
            grow = 0 if buf is None else min(buf.shape[0] * 3 // 2, FETCH_MAX_BYTES // ROW_BYTES)
            buf = None                                   # the old buffer goes before the new one comes
            buf = torch.empty(max(total, grow), C.NODE_FEATURE_DIM, device=dev, dtype=torch.float32)
        off_h = torch.cat([torch.zeros(1, dtype=torch.int64), ng.cumsum(0)])
        off_d = off_h.to(dev)
        sel32 = sel.to(torch.int32)
        ops.rows_fetch(self.y, self.row_off, sel32.to(dev), buf, off_d, idx_host=sel32, row_off_host=self.row_off_host,
                       out_off_host=off_h)
        self._stage = (sel, buf, buf[:total], off_d, off_h)
        return self._stage[2:]

    def slice(self, entries, device=None):
        """A new GalleryIndex holding the entries ``entries`` (host int64, ascending, no repeats) in that
        order, on ``device`` (default: this index's): every field taken by its axis (``FIELDS``) -- the rows and
        edges of those entries by their row and edge ranges, the per-entry fields by entry -- and the offsets rebuilt;
        layout, ``sc_mode``, ``_pack_gen`` and ``weights_id`` kept.  A "bf16+host" or "fp8+host" slice gets pinned
        host rows of its own.  Every field of the slice holds the parent's bytes for those entries
        (``ShardedGallery.split`` cuts an index into shards with it)."""
        ent = torch.as_tensor(entries)
        if ent.dtype != torch.int64 or ent.is_cuda or ent.dim() != 1 or ent.numel() == 0:
            raise FpmError("GalleryIndex.slice: entries must be a non-empty 1-D host int64 tensor")
        if int(ent[0]) < 0 or int(ent[-1]) >= self.G or bool((ent[1:] <= ent[:-1]).any()):
            raise FpmError("GalleryIndex.slice: entries must ascend without repeats inside [0, %d)" % self.G)
        self._check_live(ent, "GalleryIndex.slice")
        dev = self.device if device is None else torch.device(device)
        rows, row_off = _entry_ranges(self.row_off_host, ent)
        edges, edge_off = _entry_ranges(self.edge_off, ent)
        at = dict(rows=rows, edges=edges, entries=ent)
        at_d = {k: v.to(self.device) for k, v in at.items()}
        fields = dict(row_off=row_off.to(dev), edge_off=edge_off, P=None)
        for f in FIELDS:
            t = getattr(self, f.name)
            if t is not None and f.axis in at:
                fields[f.name] = _placed(f, t, self.layout, dev, (at_d if t.is_cuda else at)[f.axis])
        return GalleryIndex(sc_mode=self.sc_mode, pack_gen=self._pack_gen, weights_id=self.weights_id,
                            layout=self.layout, **fields)

    def _selection(self, select, pad_to=None):
        """Side 1 of a probe x gallery batch over the entries ``select`` (None: all), in that order,
        as DeviceBatch.from_pairs lays it out: (sel host int64, dict of batch fields).  Independent
        of the probe, so the last selection's data is kept for the next query (``pad_to``, see
        ``_gather``, is part of what is kept)."""
        sel = _select_host(self, select, "identify")
        if self._sel is not None and torch.equal(self._sel[0], sel) and self._sel[2] == pad_to:
            return self._sel[:2]
        self._sel = (sel, self._gather(sel, pad_to), pad_to)
        return self._sel[:2]

    def _gather(self, sel, pad_to=None):
        """One side's batch fields of the pairs whose graph on that side is entry sel[b] (host int64,
        checked by the caller; repeats are fine), as DeviceBatch.from_pairs lays that side out.  Reads
        and writes no cache: ``_selection`` keeps the last one-probe selection, a pair batch
        (``pair_batch``) gathers each side afresh.  ``pad_to`` (None: the selection's own largest
        keypoint count, as ever): the side's padded size, at least that count -- a part of a list laid
        out in the whole list's box (``ShardedGallery``)."""
        dev = self.device
        B = int(sel.numel())
        n2 = self.n[sel]
        nmax = int(n2.max())
        if pad_to is not None:
            if int(pad_to) < nmax:
                raise FpmError("identify: pad_to = %d below the selection's largest graph (%d keypoints)"
                               % (int(pad_to), nmax))
            nmax = int(pad_to)
        cnt = self.edge_off[sel + 1] - self.edge_off[sel]
        eo = torch.cat([torch.zeros(1, dtype=torch.int64), cnt.cumsum(0)])
        E = int(eo[-1])
        cnt_d = cnt.to(dev)
        pair = torch.repeat_interleave(torch.arange(B, device=dev), cnt_d, output_size=E)
        pos = torch.arange(E, device=dev) + (self.edge_off[sel] - eo[:-1]).to(dev)[pair]
        shift = (pair * nmax).to(torch.int32)
        sel_d = sel.to(dev)
        f = dict(n=n2, nmax=nmax, edge_off=eo, src=(self.src[pos] + shift).contiguous(),
                 dst=(self.dst[pos] + shift).contiguous(), pseudo=self.pseudo[pos].contiguous(),
                 w=self.w[sel_d].contiguous(), idx=sel_d.to(torch.int32).contiguous(), idx_host=sel.to(torch.int32),
                 ord2=None)
        if ORDER_ON and nmax > ORDER_MIN_NMAX and self.P is not None:
            rows = torch.repeat_interleave(torch.arange(B, device=dev), n2.to(dev).long(), output_size=int(n2.sum()))
            first = torch.cat([torch.zeros(1, dtype=torch.int64), n2.long().cumsum(0)[:-1]]).to(dev)
            loc = torch.arange(rows.numel(), device=dev) - first[rows]
            P2 = torch.zeros(B, nmax, 2, device=dev, dtype=torch.float32)
            P2[rows, loc] = self.P[loc + self.row_off[sel_d][rows]]
            f["ord2"] = hilbert_order(P2, n2, nmax)
        return f


class _CachedBatch(DeviceBatch):
    """A batch one or both of whose sides live in a GalleryIndex: laid out like ``DeviceBatch.from_pairs``,
    except that a cached side stages no node features: ``cached`` (a pair of model._CachedSide, None for a
    side with features of its own) names the index rows of each pair, and x is carried whole into every
    sub-batch.  A probe x gallery batch (``probe_batch``: shared side 0) has x[0] the probe's rows once,
    x[1] empty and side 1 cached; a pair batch (``pair_batch``: no shared side, repeated probes and entries
    are ordinary pairs) has both sides cached and x empty.  ``sc_mode``: the index's SplineConv arithmetic,
    which the forward follows (Net._sc_f32)."""

    def _carry(self, sub, b0, b1):
        sub.x = list(self.x)
        sub.cached = tuple(c and c.slice(b0, b1) for c in self.cached)
        sub.sc_mode = self.sc_mode

    def to(self, device, non_blocking=True):
        if torch.device(device) != self.device:
            raise FpmError("a batch over cached index rows stays on its index's device")
        return self


def _graph_side(graphs, dev):
    """One side's padded batch tensors of a list of graph dicts (as DeviceBatch.from_pairs stages
    them) -> (n host int32, nmax, x, src, dst, pseudo, edge counts)."""
    B = len(graphs)
    n = np.array([g["n"] for g in graphs], dtype=np.int32)
    nmax = int(n.max())
    X = np.zeros((B, nmax, C.NODE_FEATURE_DIM), np.float32)
    s_l, d_l, p_l = [], [], []
    for b, g in enumerate(graphs):
        X[b, :g["n"]] = g["x"]
        ei = np.asarray(g["edge_index"])
        s_l.append(ei[0] + b * nmax)
        d_l.append(ei[1] + b * nmax)
        p_l.append(np.asarray(g["pseudo"], dtype=np.float32).reshape(-1, 2))
    cnt = np.array([len(s) for s in s_l], dtype=np.int64)
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(dev)
    return (torch.from_numpy(n), nmax, to(X.reshape(B * nmax, -1), np.float32), to(np.concatenate(s_l), np.int32),
            to(np.concatenate(d_l), np.int32), to(np.concatenate(p_l), np.float32), cnt)


def spline_weights_id(net):
    """Digest of the SplineConv parameters (the weights an index's rows depend on); kept per weight
    version, so a repeated query does not hash again."""
    key = tuple(p._version for p in net.parameters())
    cached = getattr(net, "_sc_weights_id", None)
    if cached is not None and cached[0] == key:
        return cached[1]
    from . import params as P
    h = hashlib.blake2b(digest_size=16)
    sd = net.state_dict()
    for name in sorted(k for k in sd if k.startswith(P.SPLINE_PREFIX + ".")):
        h.update(name.encode())
        h.update(sd[name].detach().to("cpu", torch.float32).contiguous().numpy().tobytes())
    net._sc_weights_id = (key, h.hexdigest())
    return net._sc_weights_id[1]


def _pool_new(desc, g0, rows, off_host, dev):
    """The descriptors of a sub-batch's entries, whose packed fp32 rows ``rows`` (device) have the host offsets
    ``off_host``, into desc[g0 : g0 + entries] (nothing without ``desc``): where the enrolment loops round those
    rows to bf16 or quantise them to fp8."""
    if desc is not None:
        Bs = int(off_host.numel()) - 1
        ops.rows_pool(rows, off_host.to(dev), 0, Bs, out=desc[g0:g0 + Bs], row_off_host=off_host)


def _new_desc(descriptors, G, dev):
    """The table an enrolment with ``descriptors`` pools its G new entries into, or None."""
    return torch.empty(G, C.NODE_FEATURE_DIM, device=dev, dtype=torch.bfloat16) if descriptors else None


def _into_descriptors(what, index, descriptors):
    """An append pools the new entries exactly when the index holds descriptors; ``descriptors=True`` on an index
    without them is refused."""
    if descriptors and index.desc is None:
        raise FpmError("%s: descriptors=True, but the index holds no descriptors; pool the index first "
                       "(GalleryIndex.add_descriptors), or enrol it with descriptors=True" % what)
    return index.desc is not None


def _enroll_dicts(net, what, graphs, dev, sc_mode, batch, rows, r0, room=None, desc=None):
    """The enrolment loop of ``enroll`` and ``enroll_into``: the two SplineConv layers over the graph dicts in
    sub-batches of ``batch``, each sub-batch's ragged rows written from row ``r0`` on into ``rows``
    (``_alloc_rows`` / ``_store_rows``) -> the edges (graph-local src, dst, pseudo on the device, host counts
    per graph).  ``room``: the edges the index has room for (None: a new index).  ``desc``: (len(graphs), 768) bf16
    or None: the table each sub-batch's descriptors are pooled into (``_pool_new``)."""
    wp = net.packed(dev)
    srcs, dsts, pss, cnts, seen = [], [], [], [], 0
    for g0 in range(0, len(graphs), max(1, int(batch))):
        sub = graphs[g0:g0 + max(1, int(batch))]
        n, nmax, x0, src, dst, ps, cnt = _graph_side(sub, dev)
        Bs, nn_, E = len(sub), len(sub) * nmax, int(src.numel())
        seen += E
        _edge_room(what, seen, room)
        nv = n.to(dev)
        plan = ops.spline_plan(src, dst, ps, nn_, nmax, int(cnt.max()))
        yb = net._spline_layers(wp, sc_mode == "f32", x0, plan, E, nn_, nmax, nv)
        # padded -> ragged rows, edges back to graph-local ids (off the hot path: torch indexing)
        keep = (torch.arange(nmax, device=dev)[None, :] < nv.view(-1, 1)).reshape(-1)
        yr = yb[keep]
        r1 = r0 + int(yr.shape[0])
        if rows["y16"] is not None:
            ops.cast_bf16(yr, out=rows["y16"][r0:r1])
        if rows["y8"] is not None:
            ops.rows_quant8(yr, rows["y8"][r0:r1], rows["s8"][r0:r1])
        _pool_new(desc, g0, yr, torch.cat([torch.zeros(1, dtype=torch.int64), n.long().cumsum(0)]), dev)
        if rows["y_host"] is not None:
            rows["y_host"][r0:r1].copy_(yr, non_blocking=True)
        else:
            rows["y"][r0:r1].copy_(yr)
        r0 = r1
        shift = torch.repeat_interleave(torch.arange(Bs, device=dev) * nmax, torch.from_numpy(cnt).to(dev),
                                        output_size=E).to(torch.int32)
        srcs.append(src - shift)
        dsts.append(dst - shift)
        pss.append(ps)
        cnts.append(torch.from_numpy(cnt))
    return torch.cat(srcs), torch.cat(dsts), torch.cat(pss), torch.cat(cnts)


def _dict_tables(graphs, dev):
    """The per-graph fields of graph dicts -> (n host int32, w (G, 512) device, P (sum n, 2) device or None)."""
    n_all = torch.tensor([int(g["n"]) for g in graphs], dtype=torch.int32)
    w = torch.from_numpy(np.stack([np.asarray(g["w"], dtype=np.float32) for g in graphs])).to(dev)
    P = None
    if all("P" in g for g in graphs):
        P = torch.from_numpy(np.concatenate([np.asarray(g["P"], dtype=np.float32).reshape(-1, 2) for g in graphs])).to(dev)
    return n_all, w, P


def _empty_index(net, what, capacity, G, R, layout, dev, sc_mode, has_P, has_subject, has_desc=False):
    """An index of no entries over storage of ``capacity`` (checked against the G entries and R rows to come):
    ``enroll*(capacity=...)`` is an enrolment into it."""
    cap = _check_capacity(what, capacity, G, R)
    with torch.cuda.device(dev):
        st = _make_store(cap, layout, dev, ("P",) * has_P + ("subject",) * has_subject + ("desc",) * has_desc)
        return GalleryIndex._over(st, 0, 0, 0, sc_mode, net._pack_gen, spline_weights_id(net), layout)


def enroll(net, graphs, device, sc_mode=None, batch=256, layout="f32", subjects=None, capacity=None,
           descriptors=False):
    """``Net.enroll``: the two SplineConv layers over ``graphs`` (dicts as ``fpm.synth.make_graph``
    returns: n, x, w, edge_index, pseudo, optionally P) in sub-batches of ``batch`` graphs -> GalleryIndex.
    ``layout`` (LAYOUTS): where the rows are kept.  The bf16 copy is rounded per sub-batch on the device
    (``ops.cast_bf16``: the coarse kernels' own rounding), the fp8 rows and their scales quantised per sub-batch
    (``ops.rows_quant8``); for "bf16+host" and "fp8+host" each sub-batch's fp32 rows go straight to the pinned
    host tensor, so the device holds the bf16 or fp8 rows plus one sub-batch at most.
    ``subjects``: one integer label >= 0 per graph (``GalleryIndex.subject``), checked before any GPU work;
    every other field of the index is the same with or without it.  ``capacity``: (entries, keypoints[,
    edges]), the storage to enrol into (``GalleryIndex.reserve``'s sizes), for an index that will grow.
    ``descriptors``: also pool each entry's prescreen descriptor (``GalleryIndex.desc``; ``ops.rows_pool`` over each
    sub-batch's fp32 rows, the bits ``GalleryIndex.add_descriptors`` gives)."""
    sc_mode = _check_enroll(net, "enroll", layout, sc_mode)
    dev = torch.device(device)
    graphs = list(graphs)
    if not graphs:
        raise FpmError("enroll: empty gallery")
    if subjects is not None:
        subjects = _check_subjects("enroll", subjects, len(graphs))
    total = sum(int(g["n"]) for g in graphs)
    if capacity is not None:
        index = _empty_index(net, "enroll", capacity, len(graphs), total, layout, dev, sc_mode,
                             all("P" in g for g in graphs), subjects is not None, bool(descriptors))
        enroll_into(net, index, graphs, batch=batch, subjects=subjects, what="enroll")
        index.generation, index._pack_gen = 0, net._pack_gen    # a new index: as the constructor call below records it
        return index
    with torch.cuda.device(dev):
        rows = _alloc_rows(layout, dev, total)
        desc = _new_desc(descriptors, len(graphs), dev)
        src, dst, ps, cnt = _enroll_dicts(net, "enroll", graphs, dev, sc_mode, batch, rows, 0, desc=desc)
    n_all, w, P = _dict_tables(graphs, dev)
    row_off = torch.cat([torch.zeros(1, dtype=torch.int64), n_all.long().cumsum(0)])
    edge_off = torch.cat([torch.zeros(1, dtype=torch.int64), cnt.cumsum(0)])
    y_host = rows.pop("y_host")
    if y_host is not None:
        torch.cuda.current_stream(dev).synchronize()       # the host rows are complete before they are read
        rows["y"] = y_host
    return GalleryIndex(rows.pop("y"), row_off.to(dev), n_all, src, dst, ps, edge_off, w, P, sc_mode, net._pack_gen,
                        spline_weights_id(net), layout=layout, subject=subjects, desc=desc, **rows)


def _check_into(net, index, what):
    """The refusals of an enrolment into ``index`` that need no graphs."""
    if not isinstance(index, GalleryIndex):
        raise FpmError("%s: index must be a GalleryIndex (Net.enroll)" % what)
    index._need_capacity(what)
    _check_query(net, index, what)


def enroll_into(net, index, graphs, batch=256, subjects=None, what="enroll_into", descriptors=None):
    """``Net.enroll_into``: see there."""
    _check_into(net, index, what)
    descriptors = _into_descriptors(what, index, descriptors)
    graphs = list(graphs)
    if not graphs:
        raise FpmError("%s: no graphs" % what)
    if subjects is not None:
        subjects = _check_subjects(what, subjects, len(graphs))
    dev = index.device
    n_all, w, P = _dict_tables(graphs, dev)
    at = index._begin_append(what, len(graphs), int(n_all.sum()), subjects, P is not None)
    with torch.cuda.device(dev):
        desc = _new_desc(descriptors, len(graphs), dev)     # its own table until the commit: a failed append
        edges = _enroll_dicts(net, what, graphs, dev, index.sc_mode, batch, _store_rows(index), at[1],
                              index.capacity[2] - at[2], desc=desc)       # leaves the index's descriptors as they were
        return index._finish_append(what, at, n_all, w, P, *edges, subjects, desc=desc)


def _check_enroll(net, what, layout, sc_mode):
    """The refusals of ``enroll`` that need no graphs -> the SplineConv arithmetic to enrol with."""
    if net.training:
        raise FpmError("%s: inference only (call net.eval())" % what)
    if layout not in LAYOUTS:
        raise FpmError("%s: layout must be one of %s" % (what, LAYOUTS))
    sc_mode = sc_mode or ("f32" if net.dtype_mode == "f32" else "bf16")
    if sc_mode not in ("f32", "bf16") or (sc_mode == "bf16" and net.dtype_mode != "bf16"):
        raise FpmError("%s: sc_mode must be 'f32', or 'bf16' on a dtype='bf16' net" % what)
    return sc_mode


def _keypoint_args(what, P, n):
    """Padded keypoints and their counts, as given (arrays or tensors, host or device) -> (P (G, nmax, 2)
    fp32 tensor where it was, n host int64 (G,)); refuses an empty set and counts outside [1, nmax]."""
    P = torch.as_tensor(P)
    if P.dim() != 3 or P.shape[-1] != 2:
        raise FpmError("%s: P must be (G, nmax, 2) padded keypoints (got %s)" % (what, tuple(P.shape)))
    G, nmax = int(P.shape[0]), int(P.shape[1])
    if G == 0:
        raise FpmError("%s: empty gallery" % what)
    n_h = torch.as_tensor(n).reshape(-1).cpu().to(torch.int64)
    if n_h.numel() != G:
        raise FpmError("%s: %d keypoint counts for %d graphs" % (what, n_h.numel(), G))
    if int(n_h.min()) < 1 or int(n_h.max()) > nmax:
        raise FpmError("%s: a graph of %d keypoints; counts must lie in [1, nmax = %d]"
                       % (what, int(n_h.max()) if int(n_h.max()) > nmax else int(n_h.min()), nmax))
    return P.to(torch.float32), n_h


def _feature_args(what, x, w, G, nmax):
    """Node and global features as given -> (x (G, nmax, 768) fp32 view, w (G, 512) fp32), where they were."""
    x, w = torch.as_tensor(x), torch.as_tensor(w)
    D = C.NODE_FEATURE_DIM
    if tuple(x.shape) not in ((G, nmax, D), (G * nmax, D)):
        raise FpmError("%s: x must be (%d, %d, %d) or (%d, %d) node features (got %s)"
                       % (what, G, nmax, D, G * nmax, D, tuple(x.shape)))
    if tuple(w.shape) != (G, C.GLOBAL_FEATURE_DIM):
        raise FpmError("%s: w must be (%d, %d) global features (got %s)" % (what, G, C.GLOBAL_FEATURE_DIM, tuple(w.shape)))
    return x.to(torch.float32).reshape(G, nmax, D), w.to(torch.float32)


def _device_of(device, *ts):
    """The device of a keypoint call: ``device``, else that of the first device tensor, else the current GPU."""
    if device is not None:
        return torch.device(device)
    for t in ts:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    return torch.device("cuda", torch.cuda.current_device())


def _enroll_device(net, what, P, n_h, feats, dev, sc_mode, batch, layout, stg, subjects=None, capacity=None,
                   into=None, descriptors=False):
    """The enrolment loop of ``enroll_keypoints`` / ``enroll_images`` and their ``_into`` forms -> a new
    GalleryIndex, or (``into``: an index with capacity, whose ``sc_mode`` and layout are taken) the new
    entries' numbers.  ``feats(g0, g1, m)``:
    the features of graphs [g0, g1) on the device, (x (g1 - g0, >= m, 768) fp32, w (g1 - g0, 512) fp32).  Per
    sub-batch: trim to its own largest count m (the shapes ``enroll`` runs at), the graphs on the device
    (``graphs.build_graph_batch``), the two SplineConv layers as ``enroll`` calls them, and one
    ``ops.rows_pack`` from the padded output into the index's rows (and, "fp8+host", one ``ops.rows_quant8`` of
    the packed rows), allocated once before the loop (a new
    index) or reserved (``into``: the rows past ``used``; the edge count is known only per sub-batch, so the
    index changes at the end, in ``_finish_append``)."""
    from . import graphs
    G, nmax, D = int(n_h.numel()), int(P.shape[1]), C.NODE_FEATURE_DIM
    step = max(1, int(batch))
    row_off_h = torch.cat([torch.zeros(1, dtype=torch.int64), n_h.cumsum(0)])
    total = int(row_off_h[-1])
    if into is None and capacity is not None:
        into = _empty_index(net, what, capacity, G, total, layout, dev, sc_mode, True, subjects is not None,
                            bool(descriptors))
    base, room = 0, None
    if into is not None:
        descriptors = _into_descriptors(what, into, descriptors)
        at = into._begin_append(what, G, total, subjects, True)
        sc_mode, layout, base, room = into.sc_mode, into.layout, at[1], into.capacity[2] - at[2]
    wp = net.packed(dev)
    srcs, dsts, pss, cnts, seen = [], [], [], [], 0
    with torch.cuda.device(dev):
        row_off = row_off_h.to(dev)
        n_d = n_h.to(torch.int32).to(dev)
        rows = _alloc_rows(layout, dev, total) if into is None else _store_rows(into)
        y, y_host, y16 = rows.pop("y"), rows.pop("y_host"), rows["y16"]     # the rest goes to the constructor by name
        stage = None
        if y_host is not None:
            # one sub-batch of fp32 rows on the device, reused: the copies to the host are ordered on the stream
            stage = torch.empty(max(int(row_off_h[min(G, g0 + step)] - row_off_h[g0]) for g0 in range(0, G, step)), D,
                                device=dev, dtype=torch.float32)
        w_all = torch.empty(G, C.GLOBAL_FEATURE_DIM, device=dev, dtype=torch.float32)
        desc = _new_desc(descriptors, G, dev)
        for g0 in range(0, G, step):
            g1 = min(G, g0 + step)
            Bs, nsub, nv = g1 - g0, n_h[g0:g1], n_d[g0:g1]
            m = int(nsub.max())
            xs, ws = feats(g0, g1, m)
            w_all[g0:g1] = ws
            keep = torch.arange(m, device=dev)[None, :] < nv.view(-1, 1)
            x0 = torch.where(keep[..., None], xs[:, :m], torch.zeros((), device=dev)).reshape(Bs * m, D)
            gb = graphs.build_graph_batch(P[g0:g1, :m].to(dev).contiguous(), nv, stg=stg)
            cnt = gb.edge_off_host[1:] - gb.edge_off_host[:-1]
            nn_, E = Bs * m, int(gb.src.numel())
            seen += E
            _edge_room(what, seen, room)
            plan = ops.spline_plan(gb.src, gb.dst, gb.pseudo, nn_, m, int(cnt.max()))
            yb = net._spline_layers(wp, sc_mode == "f32", x0, plan, E, nn_, m, nv)
            # padded -> ragged rows (and their bf16 copy) in one pass, into their place in the index
            r0, r1 = int(row_off_h[g0]), int(row_off_h[g1])
            ops.rows_pack(yb, nv, m, row_off[g0:g1 + 1] - r0, out32=stage if y is None else y[base + r0:base + r1],
                          out16=None if y16 is None else y16[base + r0:base + r1], n_host=nsub,
                          out_off_host=row_off_h[g0:g1 + 1] - r0)
            if rows["y8"] is not None:
                ops.rows_quant8(stage[:r1 - r0], rows["y8"][base + r0:base + r1], rows["s8"][base + r0:base + r1])
            _pool_new(desc, g0, stage[:r1 - r0] if y is None else y[base + r0:base + r1], row_off_h[g0:g1 + 1] - r0, dev)
            if y_host is not None:
                y_host[base + r0:base + r1].copy_(stage[:r1 - r0], non_blocking=True)
            srcs.append(gb.src % m)                          # edges back to graph-local ids
            dsts.append(gb.dst % m)
            pss.append(gb.pseudo)
            cnts.append(cnt)
        Pk = P if P.device == dev else P.cpu()
        keep = torch.arange(nmax, device=Pk.device)[None, :] < n_h.to(Pk.device).view(-1, 1)
        Pr = Pk[keep].to(dev)
        if into is not None:
            new = into._finish_append(what, at, n_h.to(torch.int32), w_all, Pr, torch.cat(srcs), torch.cat(dsts),
                                      torch.cat(pss), torch.cat(cnts), subjects, desc=desc)
            if capacity is None:
                return new
            into.generation, into._pack_gen = 0, net._pack_gen   # a new index: as the constructor call below records it
            return into
        edge_off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cat(cnts).cumsum(0)])
        if y_host is not None:
            torch.cuda.current_stream(dev).synchronize()   # the host rows are complete before they are read
        return GalleryIndex(y if y_host is None else y_host, row_off, n_h.to(torch.int32), torch.cat(srcs),
                            torch.cat(dsts), torch.cat(pss), edge_off, w_all, Pr, sc_mode, net._pack_gen,
                            spline_weights_id(net), layout=layout, subject=subjects, desc=desc, **rows)


def _keypoint_feats(x, w, dev):
    return lambda g0, g1, m: (x[g0:g1, :m].to(dev), w[g0:g1].to(dev))


def _image_feats(net, images, P, n_h):
    nmax = int(P.shape[1])

    def feats(g0, g1, m):
        # one side of the pair front end, a sub-batch at a time: the backbone's memory is bounded by ``batch``
        xs, gs = net.image_features([images[g0:g1]], [P[g0:g1]], [n_h[g0:g1]])
        return xs[0].view(g1 - g0, nmax, C.NODE_FEATURE_DIM), gs[0]

    return feats


def enroll_keypoints(net, P, n, x, w, device=None, sc_mode=None, batch=256, layout="f32", stg="tri", subjects=None,
                     capacity=None, descriptors=False):
    """``Net.enroll_keypoints``: see there."""
    what = "enroll_keypoints"
    sc_mode = _check_enroll(net, what, layout, sc_mode)
    if subjects is not None:
        subjects = _check_subjects(what, subjects, int(torch.as_tensor(P).shape[0]))
    P, n_h = _keypoint_args(what, P, n)
    x, w = _feature_args(what, x, w, int(P.shape[0]), int(P.shape[1]))
    dev = _device_of(device, P, x)
    return _enroll_device(net, what, P, n_h, _keypoint_feats(x, w, dev), dev, sc_mode, batch, layout, stg, subjects,
                          capacity, descriptors=descriptors)


def enroll_keypoints_into(net, index, P, n, x, w, batch=256, stg="tri", subjects=None, descriptors=None):
    """``Net.enroll_keypoints_into``: see there."""
    what = "enroll_keypoints_into"
    _check_into(net, index, what)
    if subjects is not None:
        subjects = _check_subjects(what, subjects, int(torch.as_tensor(P).shape[0]))
    P, n_h = _keypoint_args(what, P, n)
    x, w = _feature_args(what, x, w, int(P.shape[0]), int(P.shape[1]))
    dev = index.device
    return _enroll_device(net, what, P, n_h, _keypoint_feats(x, w, dev), dev, None, batch, None, stg, subjects,
                          into=index, descriptors=descriptors)


def _check_images(what, images, G):
    images = torch.as_tensor(images)
    if images.dim() != 4 or int(images.shape[0]) != G:
        raise FpmError("%s: images must be (%d, 3, H, W), one per graph (got %s)" % (what, G, tuple(images.shape)))
    return images


def enroll_images(net, images, P, n, device=None, sc_mode=None, batch=256, layout="f32", stg="tri", subjects=None,
                  capacity=None, descriptors=False):
    """``Net.enroll_images``: see there."""
    what = "enroll_images"
    net._need_backbone()
    sc_mode = _check_enroll(net, what, layout, sc_mode)
    if subjects is not None:
        subjects = _check_subjects(what, subjects, int(torch.as_tensor(P).shape[0]))
    P, n_h = _keypoint_args(what, P, n)
    images = _check_images(what, images, int(P.shape[0]))
    dev = _device_of(device, P, images)
    return _enroll_device(net, what, P, n_h, _image_feats(net, images, P, n_h), dev, sc_mode, batch, layout, stg,
                          subjects, capacity, descriptors=descriptors)


def enroll_images_into(net, index, images, P, n, batch=256, stg="tri", subjects=None, descriptors=None):
    """``Net.enroll_images_into``: see there."""
    what = "enroll_images_into"
    net._need_backbone()
    _check_into(net, index, what)
    if subjects is not None:
        subjects = _check_subjects(what, subjects, int(torch.as_tensor(P).shape[0]))
    P, n_h = _keypoint_args(what, P, n)
    images = _check_images(what, images, int(P.shape[0]))
    return _enroll_device(net, what, P, n_h, _image_feats(net, images, P, n_h), index.device, None, batch, None, stg,
                          subjects, into=index, descriptors=descriptors)


def probe_graphs(net, P, n, x=None, w=None, images=None, device=None, stg="tri"):
    """``Net.probe_graphs``: see there."""
    from . import graphs
    what = "probe_graphs"
    if (images is None) == (x is None and w is None) or (x is None) != (w is None):
        raise FpmError("%s: give the features x and w, or images (not both)" % what)
    if images is not None:
        net._need_backbone()
    P, n_h = _keypoint_args(what, P, n)
    G, nmax = int(P.shape[0]), int(P.shape[1])
    if images is None:
        x, w = _feature_args(what, x, w, G, nmax)
    else:
        images = _check_images(what, images, G)
    dev = _device_of(device, P, x, images)
    with torch.cuda.device(dev):
        if images is not None:
            xs, gs = net.image_features([images], [P], [n_h])
            x, w = xs[0].view(G, nmax, C.NODE_FEATURE_DIM), gs[0]
        x, w, P = x.to(dev), w.to(dev), P.to(dev).contiguous()
        gb = graphs.build_graph_batch(P, n_h.to(torch.int32).to(dev), stg=stg)
        ei = torch.stack([gb.src % nmax, gb.dst % nmax])           # graph-local ids
        eo = gb.edge_off_host.tolist()
    return [dict(n=int(k), x=x[g, :k], w=w[g], edge_index=ei[:, eo[g]:eo[g + 1]], pseudo=gb.pseudo[eo[g]:eo[g + 1]],
                 P=P[g, :k]) for g, k in enumerate(n_h.tolist())]


_PROBE_DTYPES = {"x": (torch.float32, np.float32), "edge_index": (torch.int32, np.int32),
                 "pseudo": (torch.float32, np.float32), "w": (torch.float32, np.float32)}


def _probe_tensors(probe, dev):
    """A probe graph dict's fields staged on ``dev`` -> (n, x (n, 768) fp32, edge_index (2, E) int32, pseudo
    (E, 2) fp32, w (512,) fp32).  The values are numpy arrays (``synth.make_graph``), host tensors or device
    tensors (``Net.probe_graphs``); a tensor on ``dev`` is taken as it is: no host round trip."""
    out = []
    for key, (dt, npdt) in _PROBE_DTYPES.items():
        v = probe[key]
        if not isinstance(v, torch.Tensor):
            v = torch.from_numpy(np.ascontiguousarray(np.asarray(v).astype(npdt, copy=False)))
        out.append(v.to(device=dev, dtype=dt))
    x, ei, ps, w = out
    return int(probe["n"]), x.contiguous(), ei, ps.reshape(-1, 2), w.reshape(-1)


def probe_batch(probe, index, select=None, pad_to=None):
    """The probe x gallery batch of one probe graph over ``index`` -> (_CachedBatch, sel host int64).
    ``pad_to``: the gallery side's padded size (``GalleryIndex._gather``; None: the selection's own)."""
    dev = index.device
    sel, f = index._selection(select, pad_to)
    n0, x0, ei, ps, w0 = _probe_tensors(probe, dev)
    B = int(sel.numel())
    e0 = int(ei.shape[1])
    shift = (torch.arange(B, device=dev, dtype=torch.int32) * n0).view(B, 1)
    src0 = (ei[0].reshape(1, e0) + shift).reshape(-1).contiguous()
    dst0 = (ei[1].reshape(1, e0) + shift).reshape(-1).contiguous()
    ps0 = ps.reshape(1, e0, 2).expand(B, e0, 2).reshape(-1, 2).contiguous()
    w0 = w0.reshape(1, -1).expand(B, -1).contiguous()
    eo0 = torch.arange(B + 1, dtype=torch.int64) * e0
    bt = _CachedBatch(B, np.full(B, n0, np.int32), f["n"], [x0, x0.new_empty(0, C.NODE_FEATURE_DIM)], [w0, f["w"]],
                      [src0, f["src"]], [dst0, f["dst"]], [ps0, f["pseudo"]], dev, nmax=[n0, f["nmax"]],
                      edge_off=[eo0, f["edge_off"]], shared0=True)
    if index.layout in HOST_LAYOUTS:
        # the selected entries' fp32 rows, staged on the device in selection order: pair b reads staged
        # entry b (f["idx"], top_idx and short_idx keep speaking gallery entry numbers)
        ys, off_d, off_h = index.fetch(sel)
        ar = torch.arange(B, dtype=torch.int32)
        bt.cached = (None, _CachedSide(ys, off_d, off_h, ar.to(dev), ar))
    else:
        bt.cached = (None, _CachedSide(index.y, index.row_off, index.row_off_host, f["idx"], f["idx_host"]))
    bt.sc_mode = index.sc_mode
    bt.ord2 = f["ord2"]
    return bt, sel


def _check_query(net, index, what):
    """The refusals shared by ``identify`` and ``coarse_scores``."""
    if net.training:
        raise FpmError("%s: inference only (call net.eval()); training through an index is not supported" % what)
    if not isinstance(index, GalleryIndex):
        raise FpmError("%s: index must be a GalleryIndex (Net.enroll)" % what)
    if index.sc_mode == "bf16" and net.dtype_mode != "bf16":
        raise FpmError("%s: the index holds bf16-SplineConv rows, the net runs fp32" % what)
    net.packed(index.device)
    if index.weights_id != spline_weights_id(net):
        raise FpmError("%s: the index was enrolled with other SplineConv weights (pack generation %d, net's %d); "
                       "enroll the gallery again" % (what, index._pack_gen, net._pack_gen))


COARSE_CHUNK = 4096          # entries per coarse launch: 12 MB of coefficient scratch, whatever the gallery


class _ProbeSide:
    """What ``Net._probe_rows`` reads of a batch, for a probe graph alone (no gallery side staged)."""

    def __init__(self, probe, index):
        dev = index.device
        n0, x0, ei, ps, w0 = _probe_tensors(probe, dev)
        self.device, self.sc_mode = dev, index.sc_mode
        self.nmax = [n0, n0]
        self.x = [x0]
        self.src, self.dst = [ei[0].contiguous()], [ei[1].contiguous()]
        self.pseudo = [ps.contiguous()]
        self.edge_off = [torch.tensor([0, int(ei.shape[1])], dtype=torch.int64)]
        self.n = [torch.tensor([n0], dtype=torch.int32, device=dev)]
        self.w0 = w0.reshape(1, -1)


COARSE_ROUTES = ("fused", "wide", "auto", "stream", "any")


def _check_shortlist(shortlist, what):
    M = int(shortlist)
    if not 1 <= M <= ops.RANK_SELECT_KMAX:
        raise FpmError("%s: shortlist = %d outside [1, %d]" % (what, M, ops.RANK_SELECT_KMAX))
    return M


@contextlib.contextmanager
def _eager_prologue(net):
    """Cached-row forwards run their prologue eagerly: no HIP-graph capture per query batch."""
    keep = net.prologue_graph
    net.prologue_graph = 0
    try:
        yield
    finally:
        net.prologue_graph = keep


def _check_coarse(coarse, what):
    if coarse not in COARSE_ROUTES:
        raise FpmError("%s: coarse must be one of %s" % (what, COARSE_ROUTES))


def coarse_routes(n0, ng, coarse="any"):
    """The kernel of each pair of a probe of ``n0`` keypoints and entries of ``ng`` keypoints (host
    tensor), by number (its place in ``ops.COARSE_KERNELS``): 0 fused, 1 wide, 2 stream -> host int64
    tensor.  ``n0``: one probe's count, or (a pair list) a host tensor of ng's length, the probe's count of
    each pair.  "fused" / "wide" /
    "stream": that kernel for every pair; "auto": fused when both sides fit COARSE_NMAX, wide otherwise;
    "any": fused when both sides fit COARSE_NMAX, wide when both fit COARSE_WIDE_NMAX, stream otherwise.
    The route depends on the pair alone (its larger side).  Refuses what the route's largest kernel
    does not take."""
    _check_coarse(coarse, "coarse_scores")
    ng = torch.as_tensor(ng).view(-1).long().cpu()
    n0 = torch.as_tensor(n0).view(-1).long().cpu()
    if n0.numel() not in (1, ng.numel()):
        raise FpmError("coarse_routes: n0 must be one count or one per pair (%d for %d pairs)" % (n0.numel(), ng.numel()))
    _check_route_bounds(max(int(n0.max()), int(ng.max())), min(int(n0.min()), int(ng.min())), coarse)
    if coarse in ("fused", "wide", "stream"):
        return torch.full_like(ng, ops.COARSE_KERNELS.index(coarse))
    side = torch.maximum(ng, n0.expand_as(ng))                   # the pair's larger side
    rt = (side > ops.COARSE_NMAX).long()
    if coarse == "any":
        rt += (side > ops.COARSE_WIDE_NMAX).long()
    return rt


def _check_route_bounds(top, low, coarse):
    """The refusals of ``coarse_routes`` from the largest and the smallest graph of the query."""
    if coarse == "fused":
        if top > ops.COARSE_NMAX or low < 1:
            raise FpmError("coarse_scores: a graph of %d keypoints; the coarse pass takes boxes up to COARSE_NMAX = %d "
                           "(identify without a shortlist has no such bound)" % (top, ops.COARSE_NMAX))
    elif coarse in ("wide", "auto"):
        if top > ops.COARSE_WIDE_NMAX or low < 1:
            raise FpmError("coarse_scores: a graph of %d keypoints; the wide coarse pass takes boxes up to "
                           "COARSE_WIDE_NMAX = %d (identify without a shortlist has no such bound)"
                           % (top, ops.COARSE_WIDE_NMAX))
    elif top > ops.COARSE_STREAM_NMAX or low < 1:
        raise FpmError("coarse_scores: a graph of %d keypoints; the streamed coarse pass takes boxes up to "
                       "COARSE_STREAM_NMAX = %d (identify without a shortlist has no such bound)"
                       % (top, ops.COARSE_STREAM_NMAX))


def _launch_by_route(rt, cf, dst, launch):
    """One chunk of a coarse pass, its pairs' routes ``rt`` (``coarse_routes``, host), coefficient rows ``cf``
    and scores ``dst`` (device): ``launch(kernel, pos, pos_d, cf, dst)`` scores the chunk's pairs at positions
    ``pos`` (a host index, ``pos_d`` the same on the device) with ``kernel`` of ``ops.COARSE_KERNELS``.  One
    launch over the whole chunk (the index is the full slice: views, no copies) when every pair takes the
    same kernel; else each kernel's pairs with their coefficient rows gathered, the scores scattered back."""
    kinds = torch.unique(rt).tolist()
    if len(kinds) == 1:
        launch(ops.COARSE_KERNELS[kinds[0]], slice(None), slice(None), cf, dst)
        return
    for route in kinds:
        pos = torch.nonzero(rt == route).view(-1)
        pos_d = pos.to(cf.device)
        part = torch.empty(int(pos.numel()), device=cf.device, dtype=torch.float32)
        launch(ops.COARSE_KERNELS[route], pos, pos_d, cf[pos_d].contiguous(), part)
        dst[pos_d] = part


def _coef_rows(wp, w_probe, w_entry, coef):
    """The forward's own affinity coefficients of a chunk's pairs, from the global features of each
    pair's probe and entry ((B, 512) each), into the first B rows of the chunk's scratch ``coef`` -> those
    rows (the one-probe pass and the pair-list pass compute the same rows)."""
    cf = coef[:w_probe.shape[0]]
    ops.coef_tanh(ops.global_weights(w_probe, w_entry), wp["aff_wT"], wp["aff_b"], cf)
    return cf


def _coarse_one(net, wp, probe, index, sel, sel_d, out, chunk, coarse="fused"):
    """One probe's coarse scores over the entries ``sel`` into ``out`` (len(sel),).  ``coarse``: the
    route (``coarse_routes``; host copy of n: no synchronisation)."""
    rt = coarse_routes(int(probe["n"]), index.n[sel], coarse)
    ps = _ProbeSide(probe, index)
    yp = net._probe_rows(wp, ps)
    sel32 = sel.to(torch.int32)
    # the bf16 copy of the rows when the index keeps one: half the bytes, the same operands; the fp8 rows and
    # their scales of an "fp8+host" index
    rows, row_scale = index.coarse_rows()
    B = int(sel.numel())
    step = max(1, int(chunk))
    coef = torch.empty(min(B, step), C.NODE_FEATURE_DIM, device=index.device, dtype=torch.float32)
    w0 = ps.w0.expand(min(B, step), -1).contiguous()
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)

        def launch(kernel, pos, pos_d, cf, dst):
            ops._coarse_score_op(kernel, rows, index.row_off, sel_d[b0:b1][pos_d].contiguous(), yp, cf, C.SK_ITER_NUM,
                                 net.tau, dst, sel32[b0:b1][pos], index.row_off_host, None, row_scale)

        cf = _coef_rows(wp, w0[:b1 - b0], index.w[sel_d[b0:b1].long()], coef)
        _launch_by_route(rt[b0:b1], cf, out[b0:b1], launch)


def coarse_scores(net, probes, index, select=None, chunk=COARSE_CHUNK, coarse="fused"):
    """``Net.coarse_scores``: see there."""
    _check_coarse(coarse, "coarse_scores")
    _check_query(net, index, "coarse_scores")
    sel = _select_host(index, select, "coarse_scores")
    single = isinstance(probes, dict)
    plist = [probes] if single else list(probes)
    dev = index.device
    wp = net.packed(dev)
    out = torch.empty(len(plist), int(sel.numel()), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        sel_d = sel.to(dev).to(torch.int32).contiguous()
        for i, p in enumerate(plist):
            _coarse_one(net, wp, p, index, sel, sel_d, out[i], chunk, coarse)
    return out


IMPRESSIONS = ("all", "best")


def _check_by(what, index, by, fuse, impressions, shortlist):
    """The refusals of the subject-level arguments (before any GPU work) -> whether ``by`` is "subject"."""
    if by not in (None, "subject"):
        raise FpmError("%s: by must be None or 'subject'" % what)
    if fuse not in ops.GROUP_FUSE:
        raise FpmError("%s: fuse must be one of %s" % (what, ops.GROUP_FUSE))
    if impressions not in IMPRESSIONS:
        raise FpmError("%s: impressions must be one of %s" % (what, IMPRESSIONS))
    if by is None:
        if impressions != "all":
            raise FpmError("%s: impressions=%r without by='subject'" % (what, impressions))
        return False
    if not isinstance(index, GalleryIndex):
        raise FpmError("%s: index must be a GalleryIndex (Net.enroll)" % what)
    if index.subject is None:
        raise FpmError("%s: by='subject' needs subject labels on the index (enroll(subjects=...) or "
                       "GalleryIndex.set_subjects)" % what)
    if impressions == "best" and shortlist is None:
        raise FpmError("%s: impressions='best' needs a shortlist (the coarse score picks a subject's best impression)"
                       % what)
    return True


NORMALIZE = (None, "cohort")


def _check_open(what, subj, fuse, top_r, normalize, cohort, cohort_skip, sigma_floor, threshold):
    """The refusals of the open-set arguments (before any GPU work) -> dict: ``top_r`` (None or the r of the
    exact-stage fuse), ``stage`` (whether ``_open_set`` runs: ``normalize`` or ``threshold`` was given) and
    ``_open_set``'s arguments as ``ops.cohort_decide`` takes them."""
    isint = lambda v: isinstance(v, int) and not isinstance(v, bool)
    if top_r is not None:
        if not subj:
            raise FpmError("%s: top_r without by='subject' (it is the mean of a subject's r best impressions)" % what)
        if fuse != "mean":
            raise FpmError("%s: top_r needs fuse='mean' (got fuse=%r)" % (what, fuse))
        if not isint(top_r) or not 1 <= top_r <= ops.TOPR_MAX:
            raise FpmError("%s: top_r = %r outside [1, %d] (an integer)" % (what, top_r, ops.TOPR_MAX))
    if normalize not in NORMALIZE:
        raise FpmError("%s: normalize must be one of %s" % (what, NORMALIZE))
    if not isint(cohort) or not isint(cohort_skip) or cohort < 2 or cohort_skip < 0 \
            or cohort_skip + cohort > ops.COHORT_WINDOW:
        raise FpmError("%s: cohort = %r, cohort_skip = %r (integers, cohort >= 2, cohort_skip >= 0, cohort_skip + cohort "
                       "<= %d)" % (what, cohort, cohort_skip, ops.COHORT_WINDOW))
    floor = float(torch.tensor(float(sigma_floor), dtype=torch.float32))
    if not 0.0 < floor < float("inf"):
        raise FpmError("%s: sigma_floor must be a positive finite fp32 number (got %r)" % (what, sigma_floor))
    if threshold is not None and float(threshold) != float(threshold):
        raise FpmError("%s: threshold is NaN" % what)
    return dict(top_r=top_r, stage=normalize is not None or threshold is not None, normalize=normalize is not None,
                cohort=cohort, skip=cohort_skip, sigma_floor=sigma_floor, threshold=threshold)


def _open_set(ranked, rank, opt):
    """The open-set stage of every query form (one probe or a probe set, entries or subjects, shortlisted or
    not, with or without ``exclude_self``).  ``ranked`` (Q, X): the scores the ranking ranked -- the exact
    scores per entry, or the fused scores per subject (NaN: a subject with no pair); ``rank``: the ranking's
    result keys (top_score (Q, k), and top_subject or top_idx (Q, k): what rank 1 names); ``opt``:
    ``_check_open``'s.  ``ops.rank_select`` to the K = min(X, max(k, cohort_skip + cohort)) best -- its first k
    columns are top_score, bit for bit -- then ``ops.cohort_decide``: the cohort is the ranked list's own
    next-best candidates (with a shortlist: shortlisted candidates), NaN scores outside it.
    -> the result keys: with ``normalize`` top_z (Q, k), cohort_mu, cohort_sigma (Q,) fp32 and cohort_n (Q,)
    int32; with ``threshold`` accept (Q, k) bool -- z >= threshold, the raw score without ``normalize`` -- and
    match (Q,) int64: rank 1's subject label or entry number where it is accepted, else -1."""
    k = int(rank["top_score"].shape[1])
    K = min(int(ranked.shape[1]), max(k, opt["skip"] + opt["cohort"]))
    _, top = ops.rank_select(ranked, K)
    z, mu, sigma, n, acc = ops.cohort_decide(top, k, opt["skip"], opt["cohort"], opt["sigma_floor"], opt["threshold"],
                                             opt["normalize"])
    keys = {}
    if z is not None:
        keys.update(top_z=z, cohort_mu=mu, cohort_sigma=sigma, cohort_n=n)
    if acc is not None:
        first = rank["top_subject" if "top_subject" in rank else "top_idx"][:, 0].to(torch.int64)
        keys.update(accept=acc != 0, match=torch.where(acc[:, 0] != 0, first, torch.full_like(first, -1)))
    return keys


def _fuse_exact(scores, off_d, pos_d, fuse, top_r, off_host, pos_host):
    """The exact stage's fuse per subject: ``ops.group_scores`` with ``fuse``, or (``top_r``) the mean of each
    subject's r best impressions (``ops.group_topr``) -> (fused scores, each group's best position)."""
    if top_r is None:
        return ops.group_scores(scores, off_d, pos_d, fuse, off_host=off_host, pos_host=pos_host)
    return ops.group_topr(scores, off_d, pos_d, top_r, off_host=off_host, pos_host=pos_host)


def _subject_entry_lists(gt, spos, best=None, own=None):
    """The exact stage's entry lists of shortlisted subjects, per probe, on the host.  ``gt``: the
    selection's group tables; ``spos`` (Q, M): each probe's group numbers in coarse-rank order; ``best``
    (Q, S) or None: each group's best position (impressions "best"), None: every position of a group,
    ascending ("all"); ``own`` (Q, Gs) bool or None: positions left out (the probe's own entry)
    -> per probe (positions into the selection (L,), subject-major in the order of spos; offsets (M + 1,))."""
    off, pos = gt["off"].long(), gt["pos"].long()
    M = int(spos.shape[1])
    lists = []
    for i in range(int(spos.shape[0])):
        sp = spos[i].long()
        if best is None:
            cnt = off[sp + 1] - off[sp]
            grp = torch.repeat_interleave(torch.arange(M), cnt)
            first = torch.cat([torch.zeros(1, dtype=torch.int64), cnt.cumsum(0)])
            p = pos[off[sp][grp] + torch.arange(int(grp.numel())) - first[grp]]
        else:
            p, grp = best[i].long()[sp], torch.arange(M)
        if own is not None:
            keep = ~own[i][p]
            p, grp = p[keep], grp[keep]
        so = torch.cat([torch.zeros(1, dtype=torch.int64), torch.bincount(grp, minlength=M).cumsum(0)])
        lists.append((p, so))
    return lists


def _subject_ranking(rows, ents, offs, labels, fuse, topk, dev, top_r=None):
    """The subject ranking of the exact stage over ragged pair lists.  rows[i]: probe i's exact scores
    (L_i,) on the device; ents[i]: their entry numbers (L_i,) host; offs[i]: (M + 1,) host offsets of the M
    subjects into them; labels (Q, M) device int64.  The rows are padded with NaN to one matrix, each
    with its own group structure (``_fuse_exact``: ``ops.group_scores``, or ``ops.group_topr`` with ``top_r``),
    then ``ops.rank_topk`` over the M subjects
    -> the result keys (``_subject_keys``): subjects, subject_score (Q, M), top_subject (Q, k) int64,
    top_score (Q, k), top_idx (Q, k) int32: the entry of each top subject's best impression (-1 for a
    subject with no pair)."""
    Q = len(rows)
    L = max(1, max(int(r.numel()) for r in rows))
    mat = torch.full((Q, L), float("nan"), device=dev, dtype=torch.float32)
    ent = torch.full((Q, L), -1, dtype=torch.int32)
    for i, r in enumerate(rows):
        mat[i, :r.numel()] = r.view(-1)
        ent[i, :r.numel()] = ents[i].to(torch.int32)
    off = torch.stack([o.to(torch.int32) for o in offs])
    pos = torch.arange(L, dtype=torch.int32).view(1, L).expand(Q, L).contiguous()
    gsc, gb = _fuse_exact(mat, off.to(dev), pos.to(dev), fuse, top_r, off, pos)
    ti, ts = _rank_topk(gsc, topk)
    bp = torch.gather(gb, 1, ti.long())
    te = torch.gather(ent.to(dev), 1, bp.clamp(min=0).long())
    te = torch.where(bp >= 0, te, torch.full_like(te, -1))
    return _subject_keys(labels, gsc, ti, ts, te)


def _rank_topk(scores, topk):
    """``ops.rank_topk`` of (Q, X) scores for the ``topk`` a query asked for: k is clamped to the X entries
    or subjects there are and to the kernel's 128."""
    return ops.rank_topk(scores, max(1, min(int(topk), int(scores.shape[1]), 128)))


def _entry_ranking(scores, ent_d, topk):
    """The entry ranking of (Q, L) exact scores; ``ent_d``: the entry number of each column, (L,) shared
    by the probes or (Q, L) -> the result keys top_idx (Q, k) int32 entry numbers, top_score (Q, k)."""
    ti, ts = _rank_topk(scores, topk)
    ti = ent_d[ti.long()] if ent_d.dim() == 1 else torch.gather(ent_d, 1, ti.long())
    return dict(top_idx=ti.to(torch.int32), top_score=ts)


def _subject_keys(labels, gsc, ti, ts, te):
    """The result keys of a subject ranking: labels (Q, S) int64 the ranked subjects, gsc (Q, S) their
    fused scores, ti / ts (Q, k) ``rank_topk`` over gsc, te (Q, k) int32 each top subject's best entry."""
    return dict(subjects=labels, subject_score=gsc, top_subject=torch.gather(labels, 1, ti.long()), top_score=ts,
                top_idx=te)


def _shortlist_keys(subj, names, csc, call):
    """The result keys of the coarse stage (``_shortlist``'s names and scores, the coarse matrix)."""
    if subj:
        return dict(short_subject=names, coarse_subject_score=csc, coarse_all=call)
    return dict(short_idx=names.to(torch.int32), coarse_score=csc, coarse_all=call)


def _ragged_keys(ents, offs, dev):
    """The result keys of subject-major entry lists: short_idx the entries, short_off the subjects' (M + 1,)
    offsets into them, int32 on ``dev``."""
    return dict(short_idx=[e.to(torch.int32).to(dev) for e in ents], short_off=[o.to(torch.int32).to(dev) for o in offs])


def _attach(outs, keys):
    """The one place the query layer's keys go onto the per-probe result dicts: row i of every value
    (a (Q, ...) tensor or a list of Q tensors) to outs[i]."""
    for i, o in enumerate(outs):
        for name, v in keys.items():
            o[name] = v[i]


def _shortlist(call, sel, M, own=None, gt=None, impressions="all"):
    """The shortlist stage of every query form.  ``call`` (Q, Gs): the coarse scores of Q probes over the
    selection ``sel`` (Gs,) host int64 -- or, after a prescreen, (Q, Gs): each probe's own list --; ``M``: the shortlist asked for, clamped here to what there is;
    ``own`` (Q, Gs) host bool or None: positions that count as -inf and are left out (the probe's own
    entry); ``gt``: the selection's group tables (``subject_groups``) for a shortlist of subjects -- the
    coarse scores fused per subject by max whatever the exact stage's fuse is (a subject stays in if any
    of its impressions matches) -- with ``impressions`` "all" or "best" (each subject's best by the
    coarse score); None: a shortlist of entries.  The M best by ``ops.rank_select``, copied to the host
    once: the lists shape the host-side batches of the exact stage.
    -> (ents: per probe the exact stage's entry numbers, host int64 -- (M,) in coarse-rank order, or
    subject-major in the coarse-rank order of the subjects; offs: per probe the subjects' (M + 1,) host
    offsets into ents, None for entries; names (Q, M) int64 on call's device: the shortlisted entry
    numbers or subject labels; csc (Q, M): their coarse scores)."""
    dev = call.device
    ranked = call if own is None else call.masked_fill(own.to(dev), float("-inf"))
    if gt is None:
        M = min(M, int(sel.shape[-1]) - (own is not None))
    else:
        M = min(M, int(gt["labels"].numel()))
        ranked, cb = ops.group_scores(ranked, gt["off_d"], gt["pos_d"], "max", off_host=gt["off"], pos_host=gt["pos"])
    pos, csc = ops.rank_select(ranked, M)
    if gt is None:
        names = sel.to(dev)[pos.long()] if sel.dim() == 1 else torch.gather(sel.to(dev), 1, pos.long())
        return list(names.cpu()), None, names, csc
    lists = _subject_entry_lists(gt, pos.cpu(), cb.cpu() if impressions == "best" else None, own)
    return [sel[p] for p, _ in lists], [so for _, so in lists], gt["labels_d"][pos.long()], csc


def _check_prescreen(what, index, prescreen, shortlist, by):
    """The refusals of ``prescreen=K`` (before any GPU work) -> K, or None without a prescreen."""
    from .sharded_gallery import ShardedGallery
    if prescreen is None:
        return None
    if isinstance(index, ShardedGallery):
        raise FpmError("%s: prescreen is not supported over a ShardedGallery" % what)
    if shortlist is None:
        raise FpmError("%s: prescreen needs a shortlist (it narrows the coarse pass of shortlist=M)" % what)
    if isinstance(prescreen, bool) or not isinstance(prescreen, int) or prescreen < int(shortlist):
        raise FpmError("%s: prescreen = %r must be an integer >= shortlist = %d" % (what, prescreen, int(shortlist)))
    if by is not None:
        raise FpmError("%s: prescreen with by=%r is not supported (the group tables would differ from probe to probe)"
                       % (what, by))
    if isinstance(index, GalleryIndex) and index.desc is None:
        raise FpmError("%s: prescreen needs descriptors on the index: GalleryIndex.add_descriptors(), or "
                       "enroll*(descriptors=True)" % what)
    return prescreen


def _prescreen(dq, index, sel, K, own=None):
    """The prescreen stage: ``ops.desc_score`` of the probes' descriptors ``dq`` (Q, 768) bf16 over the selection
    ``sel`` (Gs,) host int64 of an index with descriptors, ``own`` (Q, Gs) host bool or None: positions that count
    as -inf (the probe's own entry), ``ops.rank_keep`` to the K best, K clamped to the candidates there are
    -> (lists (Q, K) host int64: each probe's entry numbers in the selection's order, the same as int32 on the
    device, their descriptor scores (Q, K))."""
    dev = index.device
    sel32 = sel.to(torch.int32)
    sel_d = sel32.to(dev)
    sc = ops.desc_score(dq, index.desc, sel_d, idx_host=sel32)
    if own is not None:
        sc = sc.masked_fill(own.to(dev), float("-inf"))
    K = max(1, min(int(K), int(sel.numel()) - (own is not None)))
    keep = ops.rank_keep(sc, K).long()
    pre_idx = sel_d[keep]
    return pre_idx.long().cpu(), pre_idx, torch.gather(sc, 1, keep)


def _check_eager(net, what):
    """The refusals of every forward over cached rows (``identify``, and the probe-set calls)."""
    if net.training:
        raise FpmError("%s: inference only (call net.eval()); training through an index is not supported" % what)
    if net.use_graphs:
        raise FpmError("%s: cached-gallery forwards are eager; switch HIP-graph replay (use_graphs) off" % what)


def identify(net, probes, index, topk=10, select=None, score="cls_prob", chunks=None, shortlist=None,
             coarse="fused", by=None, fuse="max", impressions="all", top_r=None, normalize=None, cohort=32,
             cohort_skip=1, sigma_floor=1e-6, threshold=None, coarse_all=True, prescreen=None):
    """``Net.identify``: see there."""
    from .sharded_gallery import ShardedGallery, identify_sharded
    K = _check_prescreen("identify", index, prescreen, shortlist, by)
    if isinstance(index, ShardedGallery):
        return identify_sharded(net, probes, index, topk=topk, select=select, score=score, chunks=chunks,
                                shortlist=shortlist, coarse=coarse, by=by, fuse=fuse, impressions=impressions,
                                top_r=top_r, normalize=normalize, cohort=cohort, cohort_skip=cohort_skip,
                                sigma_floor=sigma_floor, threshold=threshold, coarse_all=coarse_all)
    if coarse_all is not True:
        raise FpmError("identify: coarse_all is a keyword of the query over a ShardedGallery")
    _check_coarse(coarse, "identify")
    subj = _check_by("identify", index, by, fuse, impressions, shortlist)
    opt = _check_open("identify", subj, fuse, top_r, normalize, cohort, cohort_skip, sigma_floor, threshold)
    _check_eager(net, "identify")
    if score not in SCORES:
        raise FpmError("identify: score must be one of %s" % (SCORES,))
    _check_query(net, index, "identify")
    single = isinstance(probes, dict)
    plist = [probes] if single else list(probes)
    dev = index.device
    if shortlist is not None:
        M = _check_shortlist(shortlist, "identify")
        sel = _select_host(index, select, "identify")
        gt = index.subject_groups(sel) if subj else None
        if not plist:
            return []
        pre = {}
        if K is not None:
            # the probes' descriptors from their own rows, the K best entries of each by descriptor score, and the
            # coarse pass over each probe's own K entries and no others
            wp = net.packed(dev)
            with torch.cuda.device(dev):
                dq = torch.empty(len(plist), C.NODE_FEATURE_DIM, device=dev, dtype=torch.bfloat16)
                for i, p in enumerate(plist):
                    yp = net._probe_rows(wp, _ProbeSide(p, index))
                    one = torch.tensor([0, int(yp.shape[0])], dtype=torch.int64)
                    ops.rows_pool(yp, one.to(dev), 0, 1, out=dq[i:i + 1], row_off_host=one)
                sel, pre_idx, pre_score = _prescreen(dq, index, sel, K)
                call = torch.empty(len(plist), int(sel.shape[1]), device=dev, dtype=torch.float32)
                for i, p in enumerate(plist):
                    _coarse_one(net, wp, p, index, sel[i], pre_idx[i].contiguous(), call[i], COARSE_CHUNK, coarse)
            pre = dict(pre_idx=pre_idx, pre_score=pre_score)
        else:
            call = coarse_scores(net, plist, index, select=sel, coarse=coarse)
        with torch.cuda.device(dev):
            ents, offs, names, csc = _shortlist(call, sel, M, gt=gt, impressions=impressions)
        # the exact stage, a probe at a time: the plain ``identify`` over its list alone, in that order
        outs = [identify(net, p, index, topk=topk, select=e, score=score, chunks=chunks) for p, e in zip(plist, ents)]
        keys = _shortlist_keys(subj, names, csc, call)
        keys.update(pre)
        with torch.cuda.device(dev):
            if subj:
                keys.update(_subject_ranking([o[score] for o in outs], ents, offs, names, fuse, topk, dev, top_r))
                keys.update(_ragged_keys(ents, offs, dev))
            if opt["stage"] and subj:
                keys.update(_open_set(keys["subject_score"], keys, opt))
            elif opt["stage"]:
                # the entry ranking is each probe's own (the plain ``identify`` above): its keys, stacked
                rank = {key: torch.stack([o[key] for o in outs]) for key in ("top_idx", "top_score")}
                keys.update(_open_set(torch.stack([o[score].view(-1) for o in outs]), rank, opt))
        _attach(outs, keys)
        return outs[0] if single else outs
    outs, sel = [], None
    with _eager_prologue(net), torch.cuda.device(dev):
        for p in plist:
            bt, sel = probe_batch(p, index, select)
            outs.append(net.run(bt, chunks=chunks))
        if outs:
            sc = torch.stack([o[score].view(-1) for o in outs])
            ent_d = index._sel[1]["idx"]
            if subj:
                # one structure for all probes: the selection's groups, positions in selection order
                gt = index.subject_groups(sel)
                gsc, gb = _fuse_exact(sc, gt["off_d"], gt["pos_d"], fuse, top_r, gt["off"], gt["pos"])
                ti, ts = _rank_topk(gsc, topk)
                labs = gt["labels_d"].view(1, -1).expand(len(outs), -1)
                keys = _subject_keys(labs, gsc, ti, ts, ent_d[torch.gather(gb, 1, ti.long()).long()])
            else:
                keys = _entry_ranking(sc, ent_d, topk)
            if opt["stage"]:
                keys.update(_open_set(gsc if subj else sc, keys, opt))
            _attach(outs, keys)
    return outs[0] if single else outs


# ---- probe sets: many probes against an enrolled gallery at once -----------------------------------
COARSE_PAIRS_CHUNK = 16384   # pairs per coarse launch: 48 MB of coefficient scratch, whatever the two sets


def _check_probe_set(probes, index, what):
    """A probe set: an index enrolled from the probe graphs, its fp32 rows on the gallery's device,
    made by the same SplineConv arithmetic and weights as the gallery."""
    if not isinstance(probes, GalleryIndex):
        raise FpmError("%s: probes must be a probe set: a GalleryIndex enrolled from the probe graphs (Net.enroll)"
                       % what)
    if probes.layout in HOST_LAYOUTS:
        raise FpmError("%s: the probe set's layout is %r; a probe set keeps its fp32 rows on the device "
                       "(layout 'f32' or 'f32+bf16')" % (what, probes.layout))
    if probes.device != index.device:
        raise FpmError("%s: the probe set is on device %s, the gallery on %s" % (what, probes.device, index.device))
    if probes.sc_mode != index.sc_mode:
        raise FpmError("%s: the probe set was enrolled with sc_mode %r, the gallery with %r"
                       % (what, probes.sc_mode, index.sc_mode))
    if probes.weights_id != index.weights_id:
        raise FpmError("%s: the probe set and the gallery were enrolled with different SplineConv weights (weights_id); "
                       "enroll them with the same net" % what)


def _check_many(net, probes, index, what):
    """The refusals shared by ``match_pairs``, ``coarse_scores_many`` and ``identify_many``: the probe
    set's own (they need no net), then those of ``identify``."""
    from .sharded_gallery import ShardedGallery
    if isinstance(index, ShardedGallery) or isinstance(probes, ShardedGallery):
        raise FpmError("%s: not supported over a ShardedGallery (probe sets over shards are not built; query it "
                       "with identify(probes, sharded, shortlist=M))" % what)
    if not isinstance(index, GalleryIndex):
        raise FpmError("%s: index must be a GalleryIndex (Net.enroll)" % what)
    _check_probe_set(probes, index, what)
    _check_eager(net, what)
    _check_query(net, index, what)


def pair_batch(probes, index, pairs):
    """The batch of the pair list ``pairs`` ((B, 2) host int64: probe number, entry number, both in
    range) over a probe set and a gallery index -> _CachedBatch.  On a "bf16+host" or "fp8+host" gallery the distinct
    entries' fp32 rows are fetched and the pairs renumbered to the staging buffer."""
    dev = index.device
    q, g = pairs[:, 0].contiguous(), pairs[:, 1].contiguous()
    f0, f1 = probes._gather(q), index._gather(g)
    B = int(q.numel())
    empty = torch.empty(0, C.NODE_FEATURE_DIM, device=dev, dtype=torch.float32)
    bt = _CachedBatch(B, f0["n"], f1["n"], [empty, empty], [f0["w"], f1["w"]], [f0["src"], f1["src"]],
                      [f0["dst"], f1["dst"]], [f0["pseudo"], f1["pseudo"]], dev, nmax=[f0["nmax"], f1["nmax"]],
                      edge_off=[f0["edge_off"], f1["edge_off"]], shared0=False)
    c0 = _CachedSide(probes.y, probes.row_off, probes.row_off_host, f0["idx"], f0["idx_host"])
    if index.layout in HOST_LAYOUTS:
        uniq, inv = torch.unique(g, return_inverse=True)
        ys, off_d, off_h = index.fetch(uniq)
        inv32 = inv.to(torch.int32).contiguous()
        c1 = _CachedSide(ys, off_d, off_h, inv32.to(dev), inv32)
    else:
        c1 = _CachedSide(index.y, index.row_off, index.row_off_host, f1["idx"], f1["idx_host"])
    bt.cached = (c0, c1)
    bt.sc_mode = index.sc_mode
    bt.ord2 = f1["ord2"]
    return bt


def _run_pairs(net, probes, index, pairs, chunks):
    with _eager_prologue(net), torch.cuda.device(index.device):
        return net.run(pair_batch(probes, index, pairs), chunks=chunks)


def match_pairs(net, probes, index, pairs, chunks=None):
    """``Net.match_pairs``: see there."""
    _check_many(net, probes, index, "match_pairs")
    pairs = torch.as_tensor(pairs, dtype=torch.int64).cpu()
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.shape[0] == 0:
        raise FpmError("match_pairs: pairs must be a non-empty list of (probe number, entry number)")
    if int(pairs[:, 0].min()) < 0 or int(pairs[:, 0].max()) >= probes.G:
        raise FpmError("match_pairs: a probe number outside [0, %d)" % probes.G)
    if int(pairs[:, 1].min()) < 0 or int(pairs[:, 1].max()) >= index.G:
        raise FpmError("match_pairs: an entry number outside [0, %d)" % index.G)
    probes._check_live(pairs[:, 0], "match_pairs (probe)")
    index._check_live(pairs[:, 1], "match_pairs")
    return _run_pairs(net, probes, index, pairs, chunks)


def _coarse_pairs_order(p0, p1, Qs, Gs):
    """The pairs at places [p0, p1) of the Qs x Gs coarse pass -> (probe position, entry position, where
    their scores go in the flattened (Qs, Gs) result; None: the slice [p0, p1) itself).  Probe-major:
    place p is pair (p // Gs, p % Gs).  Scores do not depend on the order; the entry-major alternative
    (``tools/identify_bench.py --probes``: an entry's probes on one XCD) was A/B-tested once and not kept
    (DESIGN 3a)."""
    lin = torch.arange(p0, p1, dtype=torch.int64)
    return torch.div(lin, Gs, rounding_mode="floor"), lin % Gs, None


def coarse_scores_many(net, probes, index, probe_select=None, select=None, coarse="fused"):
    """``Net.coarse_scores_many``: see there."""
    _check_coarse(coarse, "coarse_scores_many")
    _check_many(net, probes, index, "coarse_scores_many")
    psel = _select_host(probes, probe_select, "coarse_scores_many (probe_select)")
    sel = _select_host(index, select, "coarse_scores_many")
    return _coarse_many(net, probes, index, psel, sel, coarse)


def _coarse_many(net, probes, index, psel, sel, coarse):
    """The pair-list coarse pass of the probes ``psel`` (Qs,) over the entries ``sel``: (Gs,) host int64, one
    selection for all probes, or (Qs, Gs), each probe's own list (after a prescreen) -> (Qs, Gs) scores."""
    nq, ng = probes.n[psel].long(), index.n[sel.reshape(-1)].long().view(sel.shape)
    _check_route_bounds(max(int(nq.max()), int(ng.max())), min(int(nq.min()), int(ng.min())), coarse)
    dev = index.device
    wp = net.packed(dev)
    Qs, Gs = int(psel.numel()), int(sel.shape[-1])
    total = Qs * Gs
    out = torch.empty(Qs, Gs, device=dev, dtype=torch.float32)
    flat = out.view(-1)                      # pair (i, j) at i * Gs + j: a launch's pairs are one slice of it
    rows, row_scale = index.coarse_rows()
    step = max(1, int(COARSE_PAIRS_CHUNK))
    coef = torch.empty(min(total, step), C.NODE_FEATURE_DIM, device=dev, dtype=torch.float32)

    with torch.cuda.device(dev):
        for p0 in range(0, total, step):
            p1 = min(total, p0 + step)
            qi, gi, where = _coarse_pairs_order(p0, p1, Qs, Gs)
            dst = flat[p0:p1] if where is None else torch.empty(p1 - p0, device=dev, dtype=torch.float32)
            q, g = psel[qi], sel[gi] if sel.dim() == 1 else sel[qi, gi]
            rt = coarse_routes(nq[qi], ng[gi] if sel.dim() == 1 else ng[qi, gi], coarse)
            cf = _coef_rows(wp, probes.w[q.to(dev)].contiguous(), index.w[g.to(dev)].contiguous(), coef)
            q32, g32 = q.to(torch.int32), g.to(torch.int32)

            def launch(kernel, pos, pos_d, cf, dst):
                qk, gk = q32[pos].contiguous(), g32[pos].contiguous()
                ops.coarse_pairs(rows, index.row_off, gk.to(dev), probes.y, probes.row_off, qk.to(dev), cf,
                                 kernel=kernel, iters=C.SK_ITER_NUM, tau=net.tau, out=dst, gidx_host=gk,
                                 qidx_host=qk, row_off_host=index.row_off_host, qrow_off_host=probes.row_off_host,
                                 row_scale=row_scale)

            _launch_by_route(rt, cf, dst, launch)
            if where is not None:
                flat[where.to(dev)] = dst
    return out


def probe_groups(n_probe_host, pairs_per_probe, group_pairs):
    """The groups of the exact stage of ``identify_many`` -> list of lists of probe positions.  Probes
    are taken in stable ascending order of keypoint count (``n_probe_host``), so a group's padded box
    stays tight; consecutive probes share a group while the group's pairs stay within ``group_pairs``
    (``pairs_per_probe``: one count, or one per probe); a probe whose own pairs exceed ``group_pairs``
    is a group alone.  Every probe is in exactly one group; deterministic."""
    n = torch.as_tensor(n_probe_host).view(-1).long().cpu()
    P = int(n.numel())
    per = torch.as_tensor(pairs_per_probe).view(-1).long().cpu()
    if per.numel() == 1:
        per = per.expand(P)
    if per.numel() != P:
        raise FpmError("probe_groups: pairs_per_probe must be one count or one per probe")
    cap = int(group_pairs)
    if cap < 1 or (P and int(per.min()) < 1):
        raise FpmError("probe_groups: group_pairs and every probe's pair count must be at least 1")
    groups, cur, used = [], [], 0
    for i in torch.argsort(n, stable=True).tolist():
        k = int(per[i])
        if cur and used + k > cap:
            groups.append(cur)
            cur, used = [], 0
        cur.append(i)
        used += k
    if cur:
        groups.append(cur)
    return groups


def _all_lists(Q, sel, dev, own=None, gt=None):
    """The entry lists of a probe-set query without a shortlist, in ``_shortlist``'s form: every entry of
    the selection ``sel`` (subject-major when ``gt`` is given) but a probe's ``own`` -> (ents, offs, names)."""
    if gt is not None:
        S = int(gt["labels"].numel())
        lists = _subject_entry_lists(gt, torch.arange(S, dtype=torch.int32).view(1, S).expand(Q, S), None, own)
        return [sel[p] for p, _ in lists], [so for _, so in lists], gt["labels_d"].view(1, S).expand(Q, S)
    Gs = int(sel.numel())
    names = sel.to(dev).view(1, Gs).expand(Q, Gs)
    if own is not None:
        names = names[~own.to(dev)].view(Q, Gs - 1)
    return list(names.cpu()), None, names                    # the pair lists shape the host-side batches: one copy


def _exact_many(net, probes, index, psel, ents, score, chunks, group_pairs):
    """The exact stage of a probe-set query: probe psel[i] against the entries ents[i] (host int64, ragged
    from probe to probe when the lists are subjects' impressions), in groups of probes (``probe_groups``)
    whose pair lists run as one batch each (``_run_pairs``) -> (outs: per probe the batch's outputs
    sliced to its own pairs, with "group" = (group number, first pair, end pair); rows: per probe its
    ``score`` row (L_i,))."""
    per = torch.tensor([int(e.numel()) for e in ents], dtype=torch.int64)
    outs, rows = [None] * len(ents), [None] * len(ents)
    for gi, grp in enumerate(probe_groups(probes.n[psel], per, group_pairs)):
        pairs = torch.cat([torch.stack([psel[i].expand(int(per[i])), ents[i]], 1) for i in grp])
        o = _run_pairs(net, probes, index, pairs, chunks)
        Bg, b0 = int(pairs.shape[0]), 0
        for i in grp:
            b1 = b0 + int(per[i])
            d = {key: (v[b0:b1] if isinstance(v, torch.Tensor) and v.dim() >= 1 and v.shape[0] == Bg else v)
                 for key, v in o.items()}
            d["group"] = (gi, b0, b1)
            rows[i] = d[score].view(-1)
            outs[i] = d
            b0 = b1
    return outs, rows


def identify_many(net, probes, index, topk=10, shortlist=None, probe_select=None, select=None, score="cls_prob",
                  coarse="fused", chunks=None, group_pairs=1024, exclude_self=False, by=None, fuse="max",
                  impressions="all", top_r=None, normalize=None, cohort=32, cohort_skip=1, sigma_floor=1e-6,
                  threshold=None, prescreen=None):
    """``Net.identify_many``: see there.  Subject-level (``by="subject"``) the exact stage's pair lists are
    ragged (a subject has as many pairs as impressions) and the exact scores are fused over one structure
    per probe (``_subject_ranking``).  ``exclude_self`` is then leave-one-out: the probe's own entry counts
    as -inf in the coarse fuse and is left out of its pair list and of its group; its subject's other
    impressions stay, and a subject emptied that way ranks last (NaN)."""
    what = "identify_many"
    K = _check_prescreen(what, index, prescreen, shortlist, by)
    _check_coarse(coarse, what)
    subj = _check_by(what, index, by, fuse, impressions, shortlist)
    opt = _check_open(what, subj, fuse, top_r, normalize, cohort, cohort_skip, sigma_floor, threshold)
    if score not in SCORES:
        raise FpmError("%s: score must be one of %s" % (what, SCORES))
    if exclude_self and probes is not index:
        raise FpmError("%s: exclude_self leaves out the pair (q, entry q) of an index searched against itself; "
                       "pass the index as its own probe set (probes is index)" % what)
    _check_many(net, probes, index, what)
    psel = _select_host(probes, probe_select, "%s (probe_select)" % what)
    sel = _select_host(index, select, what)
    Qs, Gs = int(psel.numel()), int(sel.numel())
    dev = index.device
    if exclude_self and Gs < 2:
        raise FpmError("%s: exclude_self needs at least two selected entries" % what)
    gt = index.subject_groups(sel) if subj else None
    own = (psel.view(-1, 1) == sel.view(1, -1)) if exclude_self else None
    keys = {}
    with torch.cuda.device(dev):
        if shortlist is not None:
            M = _check_shortlist(shortlist, what)
            if K is not None:
                # the probe set's descriptors if it holds them, else its selected probes' rows pooled here; own
                # entries are out after the prescreen (K is clamped below the candidates), so none is in a list
                if probes.desc is not None:
                    dq = probes.desc[psel.to(dev)].contiguous()
                else:
                    lo, hi = int(psel.min()), int(psel.max()) + 1
                    dq = ops.rows_pool(probes.y, probes.row_off, lo, hi, row_off_host=probes.row_off_host)
                    dq = dq[(psel - lo).to(dev)].contiguous()
                lists, pre_idx, pre_score = _prescreen(dq, index, sel, K, own)
                call = _coarse_many(net, probes, index, psel, lists, coarse)
                ents, offs, names, csc = _shortlist(call, lists, M)
                keys.update(pre_idx=pre_idx, pre_score=pre_score)
            else:
                call = coarse_scores_many(net, probes, index, probe_select=psel, select=sel, coarse=coarse)
                ents, offs, names, csc = _shortlist(call, sel, M, own, gt, impressions)
            keys.update(_shortlist_keys(subj, names, csc, call))
        else:
            if own is not None and not subj and not bool((own.sum(1) == 1).all()):
                raise FpmError("%s: exclude_self without a shortlist needs every probe of probe_select exactly once "
                               "in select" % what)
            ents, offs, names = _all_lists(Qs, sel, dev, own, gt)
    # only a subject-level list can come out empty (exclude_self left out the one entry it had); an entry-level
    # list has M >= 1 entries
    if min(int(e.numel()) for e in ents) < 1:
        raise FpmError("%s: a probe is left with no pair (exclude_self took its only shortlisted entry); "
                       "raise shortlist or widen select" % what)
    outs, rows = _exact_many(net, probes, index, psel, ents, score, chunks, group_pairs)
    with torch.cuda.device(dev):
        if subj:
            keys.update(_subject_ranking(rows, ents, offs, names, fuse, topk, dev, top_r))
            keys.update(_ragged_keys(ents, offs, dev))
        else:
            keys.update(_entry_ranking(torch.stack(rows), names, topk))
        if opt["stage"]:
            keys.update(_open_set(keys["subject_score"] if subj else torch.stack(rows), keys, opt))
    _attach(outs, keys)
    return outs
