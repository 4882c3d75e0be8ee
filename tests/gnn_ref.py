"""Float64 references and hand-built inputs for the association-graph GNN layer and the readout
(csrc/gnn.hip).  Plain module: no GPU, no library.

Layout, as the kernel's: a pair's state is X[c][d][i] (d = graph-2 node, i = graph-1 node, i fastest);
the references work on x (N, C) with p = d * n1max + i, N = n1max * n2max, over the WHOLE box: the
diagonal term is masked in padded p-space (p < n1b * n2b), so it reads padded positions.

The graphs are directed neighbour lists: list ``l[i]`` holds the sources of the edges into ``i``
(edges a -> i for a in l[i]); ``_graphs`` builds them so that the shapes the kernel can go wrong at
are certain to occur (see its docstring)."""
import functools

import torch

import oracle as O

# (n1max, n2max, n1 per pair, n2 per pair)
SHAPES = {
    "40x24": (40, 24, (40, 33, 13), (24, 19, 9)),
    "40x40": (40, 40, (40, 33, 13), (40, 35, 9)),
    "64x24": (64, 24, (64, 57, 13), (24, 19, 9)),
    "64x40": (64, 40, (64, 57, 13), (40, 35, 9)),
    "256x256": (256, 256, (256, 200), (256, 131)),
}

# the stage tests' boxes (tests/test_gnn_stages.py): the first four above and
STAGE_SHAPES = {k: SHAPES[k] for k in ("40x24", "40x40", "64x24", "64x40")}
STAGE_SHAPES.update({
    # nine pairs: the second round of the pair-to-XCD mapping, with 7 padded pairs in it
    "16x12x9": (16, 12, (16, 15, 14, 13, 16, 15, 14, 13, 15), (12, 11, 10, 9, 9, 10, 11, 12, 10)),
    "24x40": (24, 40, (24, 19, 13), (40, 35, 9)),            # n1max < n2max
    "65x24": (65, 24, (65, 57, 13), (24, 19, 9)),            # one lane into a second wave
    "256x24": (256, 24, (256, 200), (24, 9)),                # top of the resident form
    "257x24": (257, 24, (257, 200), (24, 9)),                # first box on form 0 by default, 320 threads
    "600x16": (600, 16, (600, 431), (16, 9)),                # the model's UNIV_SIZE cap
    "1024x16": (1024, 16, (1024, 700), (16, 9)),             # the ABI's cap; 17-channel LDS 80 KiB
})
# SHAPES stays the resident test's five boxes; 260x24 only checks the two aggregation forms on the CPU
ALL_SHAPES = dict(SHAPES, **STAGE_SHAPES)
ALL_SHAPES["260x24"] = (260, 24, (260, 200), (24, 9))

EXPLICIT_MAX = 65        # boxes up to this many keypoints aggregate over the materialised pattern
U = 2.0 ** -24           # fp32 unit roundoff


def _csr(lists, nmax):
    """Batch CSR of per-pair neighbour lists: ptr (B * nmax + 1, global, non-decreasing), nbr (local ids)."""
    ptr, nbr = [0], []
    for pair in lists:
        assert len(pair) == nmax
        for row in pair:
            assert row == sorted(set(row))
            nbr += row
            ptr.append(len(nbr))
    return torch.tensor(ptr, dtype=torch.int32), torch.tensor(nbr + [0], dtype=torch.int32)


def _pick(g, n, k):
    return sorted(torch.randperm(n, generator=g)[:k].tolist())


@functools.lru_cache(maxsize=None)
def _graphs(shape):
    """CPU tensors (ptr1, nbr1, ptr2, nbr2, n1, n2) and the per-pair Python lists behind them."""
    n1max, n2max, n1s, n2s = ALL_SHAPES[shape]
    g = torch.Generator().manual_seed(1000 + n1max * 7 + n2max)
    l1, l2 = [], []
    for n1, n2 in zip(n1s, n2s):
        assert n1 >= 13 and n2 >= 9
        # graph 1: node 0 has no neighbour, node 1 has twelve, the rest 1..9; padded nodes none
        deg = [0, 12] + [1 + int(torch.randint(0, 9, (1,), generator=g)) for _ in range(n1 - 2)]
        l1.append([_pick(g, n1, k) for k in deg] + [[] for _ in range(n1max - n1)])
        # graph 2: node d has d % 8 neighbours (every length 0..7), shuffled over the nodes
        order = torch.randperm(n2, generator=g).tolist()
        rows = [None] * n2
        for k, d in enumerate(order):
            rows[d] = _pick(g, n2, k % 8)
        l2.append(rows + [[] for _ in range(n2max - n2)])
    ptr1, nbr1 = _csr(l1, n1max)
    ptr2, nbr2 = _csr(l2, n2max)
    return (ptr1, nbr1, ptr2, nbr2, torch.tensor(n1s, dtype=torch.int32), torch.tensor(n2s, dtype=torch.int32)), l1, l2


def edge_index(lists):
    """(2, E) int64 [sources; destinations] of one graph's in-neighbour lists: a -> i for a in l[i]."""
    src = [a for row in lists for a in row]
    dst = [i for i, row in enumerate(lists) for _ in row]
    return torch.tensor([src, dst], dtype=torch.int64).reshape(2, -1)


def drop_last_of_long(lists):
    """The lists with the last neighbour of every list of length 5 or more dropped (a mistake)."""
    return [row[:-1] if len(row) >= 5 else list(row) for row in lists]


# ---------------------------------------------------------------------------------------- weights
def param_count(C):
    return 48 * C + 321


def unpack(W, C):
    """The kernel's flat per-layer layout (GnnPack in gnn.hip; matrices [in][out]) as a dict."""
    W = W.detach().cpu()
    assert W.numel() == param_count(C)
    out, o = {}, 0
    for name, shape in (("Wl", (C, 16)), ("bl", (16,)), ("Wr", (C, 16)), ("W1", (C, 16)), ("b1", (16,)),
                        ("W2", (16, 16)), ("b2", (16,)), ("wc", (16,)), ("bc", (1,))):
        n = 1
        for s in shape:
            n *= s
        out[name] = W[o:o + n].reshape(shape)
        o += n
    assert o == W.numel()
    return out


def pack_layer(sd, l):
    """Layer l of a state dict in the kernel's flat layout, as Net.packed builds it."""
    pre = "gnn_layer_%d" % l
    parts = [sd[pre + ".conv2.lin_l.weight"].t(), sd[pre + ".conv2.lin_l.bias"], sd[pre + ".conv2.lin_r.weight"].t(),
             sd[pre + ".n_self_func.0.weight"].t(), sd[pre + ".n_self_func.0.bias"],
             sd[pre + ".n_self_func.2.weight"].t(), sd[pre + ".n_self_func.2.bias"],
             sd[pre + ".classifier.weight"], sd[pre + ".classifier.bias"]]
    return torch.cat([t.reshape(-1).float() for t in parts]).contiguous()


def random_weights(C, g, scale=0.3):
    return torch.randn(param_count(C), generator=g) * scale


# ------------------------------------------------------------------------------------------ layer
MISTAKES = ("diag_block", "swap_edges", "drop_tail", "count_no_diag", "lin_r_on_agg", "swap_ch_15_16")


def _explicit_sum_count(x, e1, e2, n1max, n2max, n1b, n2b, diag):
    """Sum and count over the materialised pattern with a given diagonal index list."""
    N = n1max * n2max
    row, col = O.kron_pattern(e1, e2, n1max, n2max, 0, 0)
    row, col = torch.cat([row, diag]), torch.cat([col, diag])
    s = torch.zeros(N, x.shape[1], dtype=x.dtype)
    s.index_add_(0, col, x[row])
    cnt = torch.zeros(N, dtype=x.dtype)
    cnt.index_add_(0, col, torch.ones(col.numel(), dtype=x.dtype))
    return s, cnt


def aggregate(x, e1, e2, n1max, n2max, n1b, n2b, explicit=None, mistake=None):
    """Mean over the association pattern.  ``explicit`` None: the materialised pattern
    (oracle.kron_pattern + oracle.pattern_mean_explicit) for boxes up to EXPLICIT_MAX keypoints, the
    factorised form above.  ``mistake``: one of the aggregation mistakes of MISTAKES."""
    N = n1max * n2max
    if explicit is None:
        explicit = max(n1max, n2max) <= EXPLICIT_MAX
    if mistake == "swap_edges":
        e1 = e1.flip(0)
    if mistake == "diag_block":
        p = torch.arange(N)
        diag = p[((p % n1max) < n1b) & ((p // n1max) < n2b)]
        s, cnt = _explicit_sum_count(x, e1, e2, n1max, n2max, n1b, n2b, diag)
        return s / cnt.clamp(min=1)[:, None]
    if mistake == "count_no_diag":
        diag = torch.arange(n1b * n2b)
        s, cnt = _explicit_sum_count(x, e1, e2, n1max, n2max, n1b, n2b, diag)
        cnt[diag] -= 1
        return s / cnt.clamp(min=1)[:, None]
    if explicit:
        row, col = O.kron_pattern(e1, e2, n1max, n2max, n1b, n2b)
        return O.pattern_mean_explicit(x, row, col, N)
    return O.pattern_mean_factorized(x, e1, e2, n1max, n2max, n1b, n2b)


def _mlps(x, agg, w, mistake=None):
    r_in = agg if mistake == "lin_r_on_agg" else x
    x1 = (agg @ w["Wl"] + w["bl"]) + r_in @ w["Wr"]
    h = torch.relu(x @ w["W1"] + w["b1"])
    x1 = x1 + torch.relu(h @ w["W2"] + w["b2"])
    return x1, x1 @ w["wc"] + w["bc"]


def ref_layer(x, e1, e2, n1max, n2max, n1b, n2b, W, C, dtype=torch.float64, explicit=None, mistake=None):
    """One pair's layer: x (N, C) -> x1 (N, 16), z (N,), S = dict(x1=(N, 16), z=(N,)).

    S is the sum of absolute values of every term entering each output (the layer's formula with
    |W|, |b|, |x|; a ReLU passes the bound of its argument on), in float64 whatever ``dtype``.
    ``dtype`` float32 gives the fp32 CPU evaluation of the same formula."""
    assert x.shape == (n1max * n2max, C)
    w = {k: v.to(dtype) for k, v in unpack(W, C).items()}
    x = x.to(dtype)
    if mistake == "swap_ch_15_16":
        x = x[:, list(range(15)) + [16, 15]]
    if mistake == "drop_tail":
        raise ValueError("drop_tail is applied to the lists (drop_last_of_long), not here")
    agg = aggregate(x, e1, e2, n1max, n2max, n1b, n2b, explicit, mistake)
    x1, z = _mlps(x, agg, w, mistake)
    wa = {k: v.double().abs() for k, v in w.items()}
    xa = x.double().abs()
    agg_a = aggregate(xa, e1, e2, n1max, n2max, n1b, n2b, explicit)
    S1 = (agg_a @ wa["Wl"] + wa["bl"]) + xa @ wa["Wr"] + ((xa @ wa["W1"] + wa["b1"]) @ wa["W2"] + wa["b2"])
    return x1, z, dict(x1=S1, z=S1 @ wa["wc"] + wa["bc"])


def degrees(l1b, l2b, n1max, n2max):
    """deg1(i) + deg2(d) at every p = d * n1max + i, as a float64 (N,) tensor."""
    d1 = torch.tensor([len(r) for r in l1b], dtype=torch.float64)
    d2 = torch.tensor([len(r) for r in l2b], dtype=torch.float64)
    return (d2[:, None] + d1[None, :]).reshape(-1)


def roundings(l1b, l2b, n1max, n2max, C):
    """K(p): the fp32 roundings on the longest path from the inputs to x1[p] (see test_gnn_stages)."""
    return degrees(l1b, l2b, n1max, n2max) + (C + 22)


# ---------------------------------------------------------------------------------------- readout
def ref_readout(X, w, bias, vpart=None, dtype=torch.float64):
    """s[b][i][d] = sum_c w[c] X[b][c][d][i] + bias, and S, the sum of the terms' absolute values.
    With ``vpart`` (B, n2max, n1max) the first 16 channels' part is taken from it:
    s = w[16] X[16] + vpart + bias."""
    X, w, bias = X.to(dtype), w.to(dtype), bias.to(dtype)
    if vpart is None:
        v = torch.einsum("c,bcdi->bdi", w, X) + bias
        S = torch.einsum("c,bcdi->bdi", w.abs(), X.abs()) + bias.abs()
    else:
        vpart = vpart.to(dtype)
        v = w[16] * X[:, 16] + vpart + bias
        S = w[16].abs() * X[:, 16].abs() + vpart.abs() + bias.abs()
    return v.transpose(1, 2).contiguous(), S.double().transpose(1, 2).contiguous()


# ------------------------------------------------------------------------------------------ chain
def chain_inputs(shape, seed):
    """Kp^T = rand on each pair's valid block, zero elsewhere: (B, 1, n2max, n1max) fp32."""
    n1max, n2max, n1s, n2s = ALL_SHAPES[shape]
    g = torch.Generator().manual_seed(seed)
    X = torch.zeros(len(n1s), 1, n2max, n1max)
    for b, (n1, n2) in enumerate(zip(n1s, n2s)):
        X[b, 0, :n2, :n1] = torch.rand(n2, n1, generator=g)
    return X


def oracle_chain(shape, X0, sd, dtype):
    """The oracle's three layers + readout per pair (oracle.gnn_layer / oracle.readout, factorised
    aggregation) in ``dtype``: the layer outputs [(B, N, 17)] * 3 and s (B, n1max, n2max)."""
    n1max, n2max, n1s, n2s = ALL_SHAPES[shape]
    _, l1, l2 = _graphs(shape)
    layers, emb = [[], [], []], []
    for b, (n1b, n2b) in enumerate(zip(n1s, n2s)):
        e1, e2 = edge_index(l1[b]), edge_index(l2[b])
        agg_fn = lambda x: O.pattern_mean_factorized(x, e1, e2, n1max, n2max, n1b, n2b)
        x = X0[b].reshape(1, -1).t().to(dtype)
        for l in range(3):
            x = O.gnn_layer(x, sd, l, agg_fn, n1max, n2max, n1b, n2b)
            layers[l].append(x)
        emb.append(x)
    s = O.readout(torch.stack(emb), sd, n2max)
    return [torch.stack(v) for v in layers], s


# ------------------------------------------------------------------------------ shared layer cases
@functools.lru_cache(maxsize=None)
def init_sd():
    from fpm import params
    return params.init_params(7)


@functools.lru_cache(maxsize=None)
def layer_case(shape, C, kind="rand"):
    """Inputs of one layer launch: fp32 X (B, C, n2max, n1max), random over the whole box (padding
    included: the padded-space diagonal reads it), the packed weights W and the readout's cls_w (17,).
    ``kind`` "rand": random packed weights at scale 0.3; "init": init_params(7), layer 0 (C = 1) or 1."""
    n1max, n2max, n1s, _ = ALL_SHAPES[shape]
    g = torch.Generator().manual_seed(C * 100 + n1max + 3 * n2max + len(n1s))
    X = torch.randn(len(n1s), C, n2max, n1max, generator=g)
    if kind == "rand":
        W, cls_w = random_weights(C, g), torch.randn(17, generator=g)
    else:
        sd = init_sd()
        W, cls_w = pack_layer(sd, 0 if C == 1 else 1), sd["classifier.weight"].reshape(-1).float().clone()
    return X, W, cls_w


def pair_x(X, b):
    """Pair b of a (B, C, n2max, n1max) state as (N, C) rows, p = d * n1max + i."""
    return X[b].reshape(X.shape[1], -1).t()


@functools.lru_cache(maxsize=None)
def layer_reference(shape, C, kind="rand"):
    """Per pair: (x1, z, S, K) of ref_layer in float64 on layer_case's fp32 values.  Computed once,
    shared by every test that needs it; callers leave it unchanged."""
    n1max, n2max, n1s, n2s = ALL_SHAPES[shape]
    X, W, _ = layer_case(shape, C, kind)
    _, l1, l2 = _graphs(shape)
    out = []
    for b, (n1b, n2b) in enumerate(zip(n1s, n2s)):
        x1, z, S = ref_layer(pair_x(X, b), edge_index(l1[b]), edge_index(l2[b]), n1max, n2max, n1b, n2b, W, C)
        out.append((x1, z, S, roundings(l1[b], l2[b], n1max, n2max, C)))
    return out
