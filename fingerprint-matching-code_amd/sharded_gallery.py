"""A gallery spread over several GPUs: shortlisted 1:N search over shards that each hold a part of it.

A ``GalleryIndex`` lives on one device, which bounds the gallery one query can search.  A ``ShardedGallery``
is a list of them (the shards, one per device; a device may repeat) with a table from each shard's local entry
numbers to *global* ones.  ``Net.identify(probes, sharded, shortlist=M, ...)`` returns what the same query over
the same gallery in one index returns, bit for bit, every entry number a global number:

  coarse    every shard scores its own entries with the coarse kernels and keeps its own min(M, G_s) best
            (``ops.rank_select``), on its own device, all shards enqueued before anything is awaited;
  merge     the shards' lists, carried to ``output_device``, merged by ``ops.topk_merge`` on ``rank_select``'s
            key with the entry's global number in the low word.  An entry beaten by fewer than M entries in
            the whole gallery is beaten by fewer than M in its own shard, so the global shortlist is inside
            the union of the shards' lists; a shard's global numbers ascend, so its local tie order is the
            global one;
  exact     the forward runs where the rows are: per probe and per shard that owns part of the list, the
            probe x gallery batch over the shard's part, padded to the largest keypoint count of the
            probe's *whole* list (``probe_batch(pad_to=...)``): a pair's outputs depend on the batch's padded
            sizes and not on the pairs around it, so the parts equal the one-index forward.  The shards run one
            after another (``Net.run`` awaits its Hungarian step);
  ranking   the per-pair outputs gathered in list order on ``output_device``, ranked, fused per subject and
            judged (open set) by the functions the one-index query uses.

Subject-level queries (``by="subject"``) need every subject's impressions inside one shard
(``split(assign="subject")``); the merge then runs over subjects, keyed by their place in the ascending list of
all labels.
"""
import torch

from . import gallery as G_
from . import ops
from ._lib import FpmError
from .gallery import GalleryIndex
from .parallel import _replica, shard_bounds

MAX_SHARDS = ops.TOPK_MERGE_SMAX
# the per-pair outputs of the exact stage that a sharded query carries (in list order, on output_device)
PAIR_KEYS = ("s", "ss", "ds_mat", "perm_mat", "k_prob", "cls_prob", "cls_logits")


def _as_device(d):
    return torch.device("cuda", d) if isinstance(d, int) else torch.device(d)


class ShardedGallery:
    """``ShardedGallery(shards, entry=None, output_device=None)``: the galleries ``shards`` (1..16
    ``GalleryIndex``, whose devices may repeat: ``split(index, [0, 0])`` is how it is tested on a one-GPU box)
    searched as one gallery of G = sum G_s entries.

    ``entry[s]``: (G_s,) host int64, the global number of each local entry of shard s: ascending inside a
    shard, distinct over all shards, together 0 .. G - 1 (they fit int32).  Default: the shards concatenated.
    ``output_device``: where the lists are merged and the results live (default: the first shard's device).

    A gallery larger than one device is enrolled part by part, each part on its own device
    (``Net.enroll(part, device)``), and the parts are passed here; ``split`` cuts an index that does fit one
    device (the convenience and test route).  The shards save and load as they do alone.

    The shards are taken as they are now: a shard with removed entries is refused (``compact`` it first), and
    a query after a shard was mutated is refused (build the ShardedGallery again); a mutable shard set is not
    built.

    Refused: no shard or more than 16; shards that differ in ``sc_mode``, ``weights_id`` or layout; some shards
    with subject labels and others without; an ``entry`` table that does not ascend, collides with another
    shard's or leaves a number out.

    Host tables: ``owner`` and ``local`` (G,) int64, the shard and the local number of every global entry;
    ``n`` (G,) int32; with labels ``subject`` (G,) int64, ``labels`` (the distinct labels, ascending),
    ``subject_owner`` / ``subject_local`` per place in ``labels`` (the first shard that holds the subject, and
    its group number there) and ``subject_split`` (whether some subject has impressions in several shards).
    Per shard on its device: ``entry_d[s]`` int32 local -> global entry, ``subject_d[s]`` int32 the shard's
    group number -> place in ``labels``."""

    def __init__(self, shards, entry=None, output_device=None):
        what = "ShardedGallery"
        shards = list(shards)
        if not 1 <= len(shards) <= MAX_SHARDS:
            raise FpmError("%s: %d shards; 1 to %d are taken" % (what, len(shards), MAX_SHARDS))
        for s in shards:
            if not isinstance(s, GalleryIndex):
                raise FpmError("%s: every shard must be a GalleryIndex (Net.enroll, GalleryIndex.slice)" % what)
        if any(s.tombstones for s in shards):
            raise FpmError("%s: a shard has removed entries; compact it first (GalleryIndex.compact)" % what)
        first = shards[0]
        for name in ("sc_mode", "weights_id", "layout"):
            if any(getattr(s, name) != getattr(first, name) for s in shards):
                raise FpmError("%s: the shards differ in %s (%s)" % (what, name, [getattr(s, name) for s in shards]))
        if len({s.subject is None for s in shards}) != 1:
            raise FpmError("%s: some shards have subject labels and others have none" % what)
        sizes = [s.G for s in shards]
        total = sum(sizes)
        if total > 2 ** 31 - 1:
            raise FpmError("%s: %d entries; global entry numbers must fit int32" % (what, total))
        if entry is None:
            starts = [sum(sizes[:i]) for i in range(len(shards))]
            entry = [torch.arange(a, a + g, dtype=torch.int64) for a, g in zip(starts, sizes)]
        entry = list(entry)
        if len(entry) != len(shards):
            raise FpmError("%s: %d entry tables for %d shards" % (what, len(entry), len(shards)))
        tables = []
        for i, (e, g) in enumerate(zip(entry, sizes)):
            e = torch.as_tensor(e)
            if e.dtype != torch.int64 or e.is_cuda or tuple(e.shape) != (g,):
                raise FpmError("%s: entry[%d] must be a host int64 tensor of shard %d's %d entries" % (what, i, i, g))
            if int(e[0]) < 0 or int(e[-1]) >= total or bool((e[1:] <= e[:-1]).any()):
                raise FpmError("%s: entry[%d] must ascend without repeats inside [0, %d)" % (what, i, total))
            tables.append(e.clone())
        owner = torch.full((total,), -1, dtype=torch.int64)
        local = torch.zeros(total, dtype=torch.int64)
        for i, e in enumerate(tables):
            if bool((owner[e] >= 0).any()):
                raise FpmError("%s: entry[%d] names a global number that shard %d holds already (the tables collide)"
                               % (what, i, int(owner[e][owner[e] >= 0][0])))
            owner[e] = i
            local[e] = torch.arange(int(e.numel()), dtype=torch.int64)
        # the tables are distinct and inside [0, G), G numbers in all: none is left out
        self.shards, self.entry, self.owner, self.local = shards, tables, owner, local
        self.devices = [s.device for s in shards]
        self.output_device = self.devices[0] if output_device is None else _as_device(output_device)
        self.sc_mode, self.weights_id, self.layout = first.sc_mode, first.weights_id, first.layout
        self.n = torch.zeros(total, dtype=torch.int32)
        for s, e in zip(shards, tables):
            self.n[e] = s.n
        self.entry_d = [e.to(torch.int32).to(s.device) for s, e in zip(shards, tables)]
        self._entry_out = [e.to(self.output_device) for e in tables]       # where a shard's coarse row goes
        self.subject = self.labels = self.subject_owner = self.subject_local = self.subject_d = None
        self.subject_split = False
        if first.subject is not None:
            self.subject = torch.zeros(total, dtype=torch.int64)
            for s, e in zip(shards, tables):
                self.subject[e] = s.subject
            self.labels = torch.unique(self.subject)                       # ascending
            S = int(self.labels.numel())
            self.subject_owner = torch.full((S,), -1, dtype=torch.int64)
            self.subject_local = torch.zeros(S, dtype=torch.int64)
            places = [torch.searchsorted(self.labels, torch.unique(s.subject)) for s in shards]
            for i in reversed(range(len(shards))):                         # the first holder is written last
                self.subject_split = self.subject_split or bool((self.subject_owner[places[i]] >= 0).any())
                self.subject_owner[places[i]] = i
                self.subject_local[places[i]] = torch.arange(int(places[i].numel()), dtype=torch.int64)
            self.subject_d = [p.to(torch.int32).to(s.device) for p, s in zip(places, shards)]
            self._labels_out = self.labels.to(self.output_device)
        self._replicas = {}                                                # device -> (the net, its replica)
        self._generation = [s.generation for s in shards]                  # the tables above describe these shards

    def _check_unchanged(self, what):
        """Refuse a query over shards that were mutated (``enroll_into``, ``remove``, ``compact``) after this
        ShardedGallery was built: its tables describe the shards as they were."""
        for i, (s, g) in enumerate(zip(self.shards, self._generation)):
            if s.generation != g:
                raise FpmError("%s: shard %d has changed since this ShardedGallery was built (generation %d, then %d); "
                               "build the ShardedGallery again" % (what, i, s.generation, g))

    @property
    def G(self):
        return int(self.owner.numel())

    def nbytes(self):
        """Device bytes held, summed over the shards (the small id tables aside)."""
        return sum(s.nbytes() for s in self.shards)

    def host_nbytes(self):
        """Host bytes held, summed over the shards."""
        return sum(s.host_nbytes() for s in self.shards)

    @staticmethod
    def split(index, devices, assign="range", output_device=None):
        """``index`` cut into one shard per element of ``devices`` with ``GalleryIndex.slice`` -> ShardedGallery
        whose global numbers are ``index``'s entry numbers.  ``assign``: "range", contiguous ranges
        (``parallel.shard_bounds``); "subject", whole subjects per shard: subject number i of the ascending
        label list goes to shard i mod S; or a (G,) host tensor of shard numbers.  Every shard must get an
        entry.  The convenience and test route: a gallery larger than one device never is one index -- enrol
        each part on its own device and pass the parts to the constructor."""
        what = "ShardedGallery.split"
        if not isinstance(index, GalleryIndex):
            raise FpmError("%s: index must be a GalleryIndex" % what)
        devices = [_as_device(d) for d in devices]
        S = len(devices)
        if not 1 <= S <= MAX_SHARDS:
            raise FpmError("%s: %d devices; 1 to %d shards are taken" % (what, S, MAX_SHARDS))
        Gn = index.G
        if isinstance(assign, str) and assign == "range":
            shard = torch.zeros(Gn, dtype=torch.int64)
            for i, (b0, b1) in enumerate(shard_bounds(Gn, S)):
                shard[b0:b1] = i
        elif isinstance(assign, str) and assign == "subject":
            if index.subject is None:
                raise FpmError("%s: assign='subject' needs subject labels on the index" % what)
            _, place = torch.unique(index.subject, return_inverse=True)
            shard = place % S
        elif isinstance(assign, torch.Tensor):
            if assign.is_cuda or assign.is_floating_point() or tuple(assign.shape) != (Gn,):
                raise FpmError("%s: assign must be a (%d,) host tensor of shard numbers" % (what, Gn))
            shard = assign.to(torch.int64)
            if int(shard.min()) < 0 or int(shard.max()) >= S:
                raise FpmError("%s: a shard number outside [0, %d)" % (what, S))
        else:
            raise FpmError("%s: assign must be 'range', 'subject' or a tensor of shard numbers" % what)
        entry = [torch.nonzero(shard == i).view(-1) for i in range(S)]
        if min(int(e.numel()) for e in entry) < 1:
            raise FpmError("%s: a shard is left without an entry (%d entries over %d shards)" % (what, Gn, S))
        return ShardedGallery([index.slice(e, d) for e, d in zip(entry, devices)], entry, output_device)

    def _replica(self, net, dev):
        """The net that runs on ``dev``: a replica sharing ``net``'s parameters with packed weights of its own
        (``parallel._replica``), one per distinct device, eager."""
        held = self._replicas.get(dev)
        if held is None or held[0] is not net:
            rep = _replica(net)
            rep.use_graphs = False
            rep._enqueue_lock = None
            self._replicas[dev] = held = (net, rep)
        rep = held[1]
        rep.regression, rep.training, rep.tau = net.regression, net.training, net.tau
        return rep


def _refuse(arg, why):
    raise FpmError("identify: %s over a ShardedGallery: %s" % (arg, why))


def identify_sharded(net, probes, sharded, topk=10, select=None, score="cls_prob", chunks=None, shortlist=None,
                     coarse="fused", by=None, fuse="max", impressions="all", top_r=None, normalize=None, cohort=32,
                     cohort_skip=1, sigma_floor=1e-6, threshold=None, coarse_all=True):
    """``Net.identify`` over a ``ShardedGallery`` (the branch of ``gallery.identify``): see the module's
    docstring for the stages.  A result dict holds the per-pair outputs PAIR_KEYS in list order and the query
    keys of the one-index call, entry numbers global; the forward's batch-level keys (the losses, ``lsa``,
    ``sk_steps``, ``Kp``, ``coef``, ``ss64``) are not carried: a list's pairs ran in several batches.
    ``coarse_all=False`` drops the (G,) row of all coarse scores."""
    what = "identify"
    G_._check_coarse(coarse, what)
    if shortlist is None:
        _refuse("shortlist=None", "a sharded gallery is searched through a shortlist; pass shortlist=M")
    if select is not None:
        _refuse("select", "a selection of entries is not built for shards")
    sharded._check_unchanged(what)
    shards = sharded.shards
    subj = G_._check_by(what, shards[0], by, fuse, impressions, shortlist)
    if subj and sharded.subject_split:
        _refuse("by='subject'", "a subject has impressions in more than one shard; cut the gallery by whole "
                                "subjects (ShardedGallery.split(assign='subject'))")
    opt = G_._check_open(what, subj, fuse, top_r, normalize, cohort, cohort_skip, sigma_floor, threshold)
    G_._check_eager(net, what)
    if score not in G_.SCORES:
        raise FpmError("identify: score must be one of %s" % (G_.SCORES,))
    M = G_._check_shortlist(shortlist, what)
    reps = [sharded._replica(net, s.device) for s in shards]
    for rep, s in zip(reps, shards):
        G_._check_query(rep, s, what)
    single = isinstance(probes, dict)
    plist = [probes] if single else list(probes)
    if not plist:
        return []
    Q, od = len(plist), sharded.output_device

    # ---- coarse: every shard's scores and its own shortlist, enqueued on its device; nothing is awaited
    calls, lists, bests = [], [], []
    for s, (rep, shard) in enumerate(zip(reps, shards)):
        call = G_.coarse_scores(rep, plist, shard, coarse=coarse)
        with torch.cuda.device(shard.device):
            if subj:
                gt = shard.subject_groups()
                ranked, cb = ops.group_scores(call, gt["off_d"], gt["pos_d"], "max", off_host=gt["off"],
                                              pos_host=gt["pos"])
                table = sharded.subject_d[s]
            else:
                ranked, cb, table = call, None, sharded.entry_d[s]
            pos, csc = ops.rank_select(ranked, min(M, int(ranked.shape[1])))
            ids = table[pos.long()]
        calls.append(call)
        lists.append((ids, csc))
        bests.append(cb)

    # ---- merge on the output device; one copy of the merged ids to the host
    with torch.cuda.device(od):
        list_off = [0]
        for ids, _ in lists:
            list_off.append(list_off[-1] + int(ids.shape[1]))
        Mm = min(M, int(sharded.labels.numel()) if subj else sharded.G)
        top_id, csc, _ = ops.topk_merge(torch.cat([c.to(od, non_blocking=True) for _, c in lists], 1),
                                        torch.cat([i.to(od, non_blocking=True) for i, _ in lists], 1), list_off, Mm)
        call_all = None
        if coarse_all:
            call_all = torch.empty(Q, sharded.G, device=od, dtype=torch.float32)
            for at, c in zip(sharded._entry_out, calls):
                call_all[:, at] = c.to(od, non_blocking=True)
        top_h = top_id.cpu().long()
        if subj:
            names = sharded._labels_out[top_id.long()]
            ents, offs = _subject_lists(sharded, top_h, [None if impressions != "best" else b.cpu() for b in bests])
        else:
            names = top_id.long()
            ents, offs = list(top_h), None

    # ---- exact: per probe, each owning shard's part in the whole list's box, gathered in list order
    outs = [_exact_sharded(reps, sharded, p, e, chunks, od) for p, e in zip(plist, ents)]

    # ---- ranking, fusion and the open-set stage: the one-index query's own functions
    keys = G_._shortlist_keys(subj, names, csc, call_all if coarse_all else [None] * Q)
    if not coarse_all:
        del keys["coarse_all"]
    with torch.cuda.device(od):
        if subj:
            keys.update(G_._subject_ranking([o[score] for o in outs], ents, offs, names, fuse, topk, od, top_r))
            keys.update(G_._ragged_keys(ents, offs, od))
            if opt["stage"]:
                keys.update(G_._open_set(keys["subject_score"], keys, opt))
        else:
            rank = [G_._entry_ranking(o[score].view(1, -1), e.to(torch.int32).to(od), topk) for o, e in zip(outs, ents)]
            keys.update({k: torch.cat([r[k] for r in rank]) for k in ("top_idx", "top_score")})
            if opt["stage"]:
                keys.update(G_._open_set(torch.stack([o[score].view(-1) for o in outs]), keys, opt))
    G_._attach(outs, keys)
    return outs[0] if single else outs


def _subject_lists(sharded, top, bests):
    """The exact stage's entry lists of the merged subjects, per probe, on the host.  ``top`` (Q, M): places
    in ``sharded.labels`` in merged order; ``bests[s]`` (Q, S_s) or None: shard s's best local entry per group
    (impressions "best"), None: every entry of a group, ascending -> (ents: per probe global entry numbers,
    subject-major in merged order; offs: per probe the subjects' (M + 1,) offsets)."""
    tables = [s.subject_groups() for s in sharded.shards]
    ents, offs = [], []
    for i in range(int(top.shape[0])):
        parts = []
        for place in top[i].tolist():
            s, g = int(sharded.subject_owner[place]), int(sharded.subject_local[place])
            gt = tables[s]
            if bests[s] is None:
                loc = gt["pos"][int(gt["off"][g]):int(gt["off"][g + 1])].long()
            else:
                loc = bests[s][i, g].long().view(1)
            parts.append(sharded.entry[s][loc])
        ents.append(torch.cat(parts))
        offs.append(torch.cat([torch.zeros(1, dtype=torch.int64),
                               torch.tensor([int(p.numel()) for p in parts], dtype=torch.int64).cumsum(0)]))
    return ents, offs


def _exact_sharded(reps, sharded, probe, ent, chunks, od):
    """One probe's exact stage over the global entries ``ent`` (host int64, in list order) -> dict of the
    PAIR_KEYS, (L, ...) each on ``od``.  Every shard that owns part of the list runs the forward over its
    part, padded to the whole list's largest keypoint count, one shard after another."""
    own = sharded.owner[ent]
    nstar = int(sharded.n[ent].max())
    out = {}
    for s in torch.unique(own).tolist():
        shard, rep = sharded.shards[s], reps[s]
        where = torch.nonzero(own == s).view(-1)
        with G_._eager_prologue(rep), torch.cuda.device(shard.device):
            bt, _ = G_.probe_batch(probe, shard, select=sharded.local[ent[where]], pad_to=nstar)
            res = rep.run(bt, chunks=chunks)
        with torch.cuda.device(od):
            where_d = where.to(od)
            for key in PAIR_KEYS:
                if key not in res:
                    continue
                v = res[key].to(od)
                if key not in out:
                    out[key] = torch.empty((int(ent.numel()),) + tuple(v.shape[1:]), device=od, dtype=v.dtype)
                out[key][where_d] = v
    return out
