"""The stored fields of a ``GalleryIndex``, one by one, through every operation that enumerates them (no GPU):
a census of all fifteen arrays after ``reserve``, ``save`` / ``load`` (with and without ``capacity``), ``slice``,
``remove`` + ``compact`` and a save with tombstones, for every layout with and without each optional field, against
plain torch indexing of the tensors the index was made from; the files ``load`` accepts and refuses, as a literal
table; and the byte counts against sums written out here.

The list of fields is written out below on purpose: it is not read from the package."""
import itertools

import pytest
import torch

from fpm import _lib, ops
from fpm.gallery import GalleryIndex

LAYOUTS = ("f32", "f32+bf16", "bf16+host", "fp8+host")
ROWS = ("y", "y16", "y8", "s8", "P")                     # one row per keypoint
EDGES = ("src", "dst", "pseudo")                         # one row per edge
ENTRIES = ("w", "desc", "n", "subject")                  # one row per entry
OFFSETS = ("row_off", "row_off_host", "edge_off")        # entries + 1
ALL = ROWS + EDGES + ENTRIES + OFFSETS
DTYPES = dict(y=torch.float32, y16=torch.bfloat16, y8=torch.float8_e4m3fn, s8=torch.float32, P=torch.float32,
              src=torch.int32, dst=torch.int32, pseudo=torch.float32, w=torch.float32, desc=torch.bfloat16,
              n=torch.int32, subject=torch.int64, row_off=torch.int64, row_off_host=torch.int64, edge_off=torch.int64)
N = (1, 3, 2, 4, 1)
CNT = (2, 0, 5, 3, 4)
SUBJECT = (3, 3, 0, 9, 0)
G, R, E = 5, 11, 14


def _u8(t):
    return t.contiguous().view(torch.uint8)


def originals(layout, P, subject, desc):
    """The tensors the index is made from -> {field: tensor or None}, every one of ALL."""
    g = torch.Generator().manual_seed(7)
    f = dict.fromkeys(ALL)
    f["n"] = torch.tensor(N, dtype=torch.int32)
    f["row_off"] = torch.tensor([0, 1, 4, 6, 10, 11], dtype=torch.int64)
    f["row_off_host"] = f["row_off"].clone()
    f["edge_off"] = torch.tensor([0, 2, 2, 7, 10, 14], dtype=torch.int64)
    f["y"] = torch.randn(R, 768, generator=g) * torch.ldexp(torch.ones(R), torch.arange(R) % 5 - 2)[:, None]
    if layout in ("f32+bf16", "bf16+host"):
        f["y16"] = f["y"].to(torch.bfloat16)
    if layout == "fp8+host":
        f["y8"], f["s8"] = ops.rows_quant8(f["y"])
    f["src"] = torch.randint(0, 4, (E,), generator=g, dtype=torch.int32)
    f["dst"] = torch.randint(0, 4, (E,), generator=g, dtype=torch.int32)
    f["pseudo"] = torch.rand(E, 2, generator=g)
    f["w"] = torch.rand(G, 512, generator=g)
    if P:
        f["P"] = torch.rand(R, 2, generator=g)
    if subject:
        f["subject"] = torch.tensor(SUBJECT, dtype=torch.int64)
    if desc:
        f["desc"] = torch.randn(G, 768, generator=g).to(torch.bfloat16)
    return f


def make(layout, f):
    c = {k: None if v is None else v.clone() for k, v in f.items()}
    return GalleryIndex(c["y"], c["row_off"], c["n"], c["src"], c["dst"], c["pseudo"], c["edge_off"], c["w"], c["P"],
                        "f32", 4, "0123abcd", y16=c["y16"], layout=layout, subject=c["subject"], y8=c["y8"], s8=c["s8"],
                        desc=c["desc"])


def expected(f, ent):
    """The fields of the entries ``ent`` (ascending), by plain indexing of the originals."""
    ro, eo = f["row_off"].tolist(), f["edge_off"].tolist()
    rows = torch.tensor([r for e in ent for r in range(ro[e], ro[e + 1])], dtype=torch.int64)
    edges = torch.tensor([k for e in ent for k in range(eo[e], eo[e + 1])], dtype=torch.int64)
    ents = torch.tensor(ent, dtype=torch.int64)
    want = dict.fromkeys(ALL)
    for names, at in ((ROWS, rows), (EDGES, edges), (ENTRIES, ents)):
        for k in names:
            if f[k] is not None:
                want[k] = _u8(f[k])[at].view(f[k].dtype) if k == "y8" else f[k][at]
    zero = torch.zeros(1, dtype=torch.int64)
    want["row_off"] = torch.cat([zero, torch.tensor([N[e] for e in ent]).cumsum(0)])
    want["row_off_host"] = want["row_off"]
    want["edge_off"] = torch.cat([zero, torch.tensor([CNT[e] for e in ent]).cumsum(0)])
    return want


def census(idx, want, what):
    for k in ALL:
        got = getattr(idx, k)
        if want[k] is None:
            assert got is None, (what, k)
            continue
        assert isinstance(got, torch.Tensor) and got.dtype == DTYPES[k] == want[k].dtype, (what, k)
        assert tuple(got.shape) == tuple(want[k].shape), (what, k)
        assert torch.equal(_u8(got) if k == "y8" else got, _u8(want[k]) if k == "y8" else want[k]), (what, k)
    assert (idx.sc_mode, idx._pack_gen, idx.weights_id) == ("f32", 4, "0123abcd"), what
    assert idx.used == (want["n"].numel(), want["y"].shape[0], want["src"].numel()), what


@pytest.mark.parametrize("desc", [False, True], ids=["", "desc"])
@pytest.mark.parametrize("subject", [False, True], ids=["", "subject"])
@pytest.mark.parametrize("P", [False, True], ids=["", "P"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_field_census(layout, P, subject, desc, tmp_path):
    f = originals(layout, P, subject, desc)
    whole, part, cap = expected(f, [0, 1, 2, 3, 4]), expected(f, [0, 2, 3]), (G + 3, R + 7, E + 5)
    idx = make(layout, f)
    census(idx, whole, "constructor")
    assert idx.layout == layout and idx.capacity is None
    roomy = idx.reserve(*cap)
    census(roomy, whole, "reserve")
    census(idx, whole, "reserve left its parent alone")
    assert roomy.capacity == cap and roomy.layout == layout and roomy.generation == 0
    for name, src in (("plain", idx), ("roomy", roomy)):
        src.save(tmp_path / "a.pt")
        back = GalleryIndex.load(tmp_path / "a.pt", "cpu")
        census(back, whole, "save, load (%s)" % name)
        assert back.capacity is None and back.layout == layout and not back.tombstones
        back = GalleryIndex.load(tmp_path / "a.pt", "cpu", capacity=cap)
        census(back, whole, "save, load(capacity=) (%s)" % name)
        assert back.capacity == cap and back.layout == layout and back.generation == 0
        cut = src.slice(torch.tensor([0, 2, 3]))
        census(cut, part, "slice (%s)" % name)
        assert cut.capacity is None and cut.layout == layout
    census(idx, whole, "after the reads")
    for name, src in (("plain", make(layout, f)), ("roomy", roomy)):
        src.remove([1, 4])
        census(src, whole, "remove (%s)" % name)
        src.save(tmp_path / "dead.pt")
        for c in (None, cap):
            back = GalleryIndex.load(tmp_path / "dead.pt", "cpu", capacity=c)
            census(back, whole, "remove, save, load (%s, %s)" % (name, c))
            assert back.removed.tolist() == [False, True, False, False, True] and back.live.tolist() == [0, 2, 3]
            assert back.capacity == c
        assert src.compact().tolist() == [0, -1, 1, 2, -1]
        census(src, part, "remove, compact (%s)" % name)
        assert src.capacity == (cap if name == "roomy" else (G, R, E)) and not src.tombstones
        for k in ALL:                                    # the fields are views of the storage the index keeps
            if part[k] is not None:
                assert getattr(src, k).data_ptr() == src._store[k].data_ptr(), (name, k)


# ------------------------------------------------------------------------------------------ what load takes
BASE = ("format", "y", "row_off", "n", "src", "dst", "pseudo", "edge_off", "w", "sc_mode", "pack_gen", "weights_id",
        "P", "subject")
ROW_KEYS = {"f32": (), "f32+bf16": ("y16",), "bf16+host": ("y16",), "fp8+host": ("y8", "s8")}


def correct_keys(fmt, layout):
    """The keys a file of ``fmt`` holds for ``layout`` as ``save`` writes them (format 1 names no layout)."""
    return BASE + (("layout",) if fmt >= 2 or layout != "f32" else ()) + ROW_KEYS[layout] + \
        (("removed",) if fmt == 3 else ()) + (("desc",) if fmt == 5 else ())


def variants(fmt, layout):
    keys = correct_keys(fmt, layout)
    out = [("as written", keys)]
    out += [("without " + k, tuple(x for x in keys if x != k)) for k in keys[len(BASE):]]
    if fmt != 5:
        out.append(("with desc", keys + ("desc",)))
    if layout != "fp8+host":
        out += [("with y8", keys + ("y8",)), ("with s8", keys + ("s8",))]
    return out


# (format, layout, variant) -> the layout of the index ``load`` returns, or None where it raises.  Recorded from
# the container before its fields were tabulated.  None is a refusal (FpmError); "KeyError" marks the files that got
# past that version's format check and failed on the missing key: those may be refused, never accepted.
LOADS = """
1 f32       | as written      -> f32
1 f32       | with desc       -> None
1 f32       | with y8         -> f32
1 f32       | with s8         -> f32
1 f32+bf16  | as written      -> f32
1 f32+bf16  | without layout  -> f32
1 f32+bf16  | without y16     -> f32
1 f32+bf16  | with desc       -> None
1 f32+bf16  | with y8         -> f32
1 f32+bf16  | with s8         -> f32
1 bf16+host | as written      -> f32
1 bf16+host | without layout  -> f32
1 bf16+host | without y16     -> f32
1 bf16+host | with desc       -> None
1 bf16+host | with y8         -> f32
1 bf16+host | with s8         -> f32
1 fp8+host  | as written      -> None
1 fp8+host  | without layout  -> f32
1 fp8+host  | without y8      -> None
1 fp8+host  | without s8      -> None
1 fp8+host  | with desc       -> None
2 f32       | as written      -> f32
2 f32       | without layout  -> KeyError
2 f32       | with desc       -> None
2 f32       | with y8         -> f32
2 f32       | with s8         -> f32
2 f32+bf16  | as written      -> f32+bf16
2 f32+bf16  | without layout  -> KeyError
2 f32+bf16  | without y16     -> KeyError
2 f32+bf16  | with desc       -> None
2 f32+bf16  | with y8         -> f32+bf16
2 f32+bf16  | with s8         -> f32+bf16
2 bf16+host | as written      -> bf16+host
2 bf16+host | without layout  -> KeyError
2 bf16+host | without y16     -> KeyError
2 bf16+host | with desc       -> None
2 bf16+host | with y8         -> bf16+host
2 bf16+host | with s8         -> bf16+host
2 fp8+host  | as written      -> None
2 fp8+host  | without layout  -> KeyError
2 fp8+host  | without y8      -> None
2 fp8+host  | without s8      -> None
2 fp8+host  | with desc       -> None
3 f32       | as written      -> f32
3 f32       | without layout  -> None
3 f32       | without removed -> None
3 f32       | with desc       -> None
3 f32       | with y8         -> f32
3 f32       | with s8         -> f32
3 f32+bf16  | as written      -> f32+bf16
3 f32+bf16  | without layout  -> None
3 f32+bf16  | without y16     -> KeyError
3 f32+bf16  | without removed -> None
3 f32+bf16  | with desc       -> None
3 f32+bf16  | with y8         -> f32+bf16
3 f32+bf16  | with s8         -> f32+bf16
3 bf16+host | as written      -> bf16+host
3 bf16+host | without layout  -> None
3 bf16+host | without y16     -> KeyError
3 bf16+host | without removed -> None
3 bf16+host | with desc       -> None
3 bf16+host | with y8         -> bf16+host
3 bf16+host | with s8         -> bf16+host
3 fp8+host  | as written      -> None
3 fp8+host  | without layout  -> None
3 fp8+host  | without y8      -> None
3 fp8+host  | without s8      -> None
3 fp8+host  | without removed -> None
3 fp8+host  | with desc       -> None
4 f32       | as written      -> None
4 f32       | without layout  -> None
4 f32       | with desc       -> None
4 f32       | with y8         -> None
4 f32       | with s8         -> None
4 f32+bf16  | as written      -> None
4 f32+bf16  | without layout  -> None
4 f32+bf16  | without y16     -> None
4 f32+bf16  | with desc       -> None
4 f32+bf16  | with y8         -> None
4 f32+bf16  | with s8         -> None
4 bf16+host | as written      -> None
4 bf16+host | without layout  -> None
4 bf16+host | without y16     -> None
4 bf16+host | with desc       -> None
4 bf16+host | with y8         -> None
4 bf16+host | with s8         -> None
4 fp8+host  | as written      -> fp8+host
4 fp8+host  | without layout  -> None
4 fp8+host  | without y8      -> None
4 fp8+host  | without s8      -> None
4 fp8+host  | with desc       -> None
5 f32       | as written      -> f32
5 f32       | without layout  -> None
5 f32       | without desc    -> None
5 f32       | with y8         -> f32
5 f32       | with s8         -> f32
5 f32+bf16  | as written      -> f32+bf16
5 f32+bf16  | without layout  -> None
5 f32+bf16  | without y16     -> None
5 f32+bf16  | without desc    -> None
5 f32+bf16  | with y8         -> f32+bf16
5 f32+bf16  | with s8         -> f32+bf16
5 bf16+host | as written      -> bf16+host
5 bf16+host | without layout  -> None
5 bf16+host | without y16     -> None
5 bf16+host | without desc    -> None
5 bf16+host | with y8         -> bf16+host
5 bf16+host | with s8         -> bf16+host
5 fp8+host  | as written      -> fp8+host
5 fp8+host  | without layout  -> None
5 fp8+host  | without y8      -> None
5 fp8+host  | without s8      -> None
5 fp8+host  | without desc    -> None
"""


def load_cases():
    for fmt, layout in itertools.product((1, 2, 3, 4, 5), LAYOUTS):
        for name, keys in variants(fmt, layout):
            yield fmt, layout, name, keys


def file_dict(fmt, layout, keys):
    f = originals("fp8+host", True, True, True)
    f["y16"] = f["y"].to(torch.bfloat16)
    f["y8"] = _u8(f["y8"])
    d = {k: f[k] for k in keys if k in f}
    extra = dict(format=fmt, sc_mode="f32", pack_gen=4, weights_id="0123abcd", layout=layout,
                 removed=torch.tensor([False, True, False, False, True]))
    d.update({k: extra[k] for k in keys if k in extra})
    return d


def outcome(d, path, capacity=None):
    torch.save(d, path)
    try:
        return GalleryIndex.load(path, "cpu", capacity=capacity).layout
    except _lib.FpmError:
        return None
    except KeyError:
        return "KeyError"


def test_load_matrix(tmp_path):
    want = {}
    for line in LOADS.strip().splitlines():
        key, val = line.split("->")
        head, name = key.split("|")
        fmt, layout = head.split()
        want[(int(fmt), layout, name.strip())] = val.strip()
    refused = lambda v: v in ("None", "KeyError")      # a file that failed on a missing key may now be refused
    for capacity in (None, (G + 3, R + 7, E + 5)):      # both branches of load take and refuse the same files
        got = {}
        for fmt, layout, name, keys in load_cases():
            got[(fmt, layout, name)] = str(outcome(file_dict(fmt, layout, keys), tmp_path / "f.pt", capacity))
            print("%d %-9s | %-15s -> %s" % (fmt, layout, name, got[(fmt, layout, name)]))
        assert sorted(got) == sorted(want)
        bad = {k: (got[k], want[k]) for k in got if (got[k] != want[k] and not (refused(got[k]) and refused(want[k])))
               or (got[k] == "KeyError" and want[k] == "None")}
        assert not bad, (capacity, bad)
        # a format 5 file that names no layout or an unknown one, and a format that is no number, are load's to refuse
        whole = file_dict(5, "f32", correct_keys(5, "f32"))
        for odd in (dict(whole, layout="bf16"), dict(whole, layout=None), dict(whole, format=[5])):
            torch.save(odd, tmp_path / "odd.pt")
            with pytest.raises(_lib.FpmError, match="is not a gallery index of format"):
                GalleryIndex.load(tmp_path / "odd.pt", "cpu", capacity=capacity)


# ------------------------------------------------------------------------------------------------ byte counts
ROW_BYTES = {"f32": 3072, "f32+bf16": 3072 + 1536, "bf16+host": 1536, "fp8+host": 768 + 4}


@pytest.mark.parametrize("layout", LAYOUTS)
def test_byte_counts(layout):
    cap = (G + 3, R + 7, E + 5)
    for desc, groups, roomy in itertools.product((False, True), (False, True), (False, True)):
        idx = make(layout, originals(layout, True, True, desc))
        if roomy:
            idx = idx.reserve(*cap)
        g, r, e = cap if roomy else (G, R, E)
        # the rows and keypoints, the edges (src, dst, pseudo), w and the device offsets
        want = r * ROW_BYTES[layout] + r * 8 + e * (4 + 4 + 8) + g * 2048 + (g + 1) * 8
        if desc:
            want += g * 1536
        if groups:
            idx.subject_groups()
            want += 3 * 8 + 4 * 4 + G * 4                # three subjects: labels, offsets, positions on the device
        assert idx.nbytes() == want, (desc, groups, roomy)
        assert idx.host_nbytes() == (r * 3072 if layout in ("bf16+host", "fp8+host") else 0), (desc, groups, roomy)
    bare = make(layout, originals(layout, False, False, False))
    assert bare.nbytes() == R * ROW_BYTES[layout] + E * 16 + G * 2048 + (G + 1) * 8
