"""Plain references of the SplineConv plan and layer (csrc/spline.hip), written from the definition
(PyG SplineConv(768, 768, dim=2, kernel_size=5, aggr='max'), open B-spline of degree 1) in numpy:
integers exactly, the basis in the kernel's single fp32 operations, everything else in float64.
Test helper only -- shared by test_spline_ref_cpu.py (which holds it to the oracle) and
test_spline_stages.py (which holds the kernels to it).

``variant`` (ref_plan / ref_combine) applies one deliberate mistake, to show that the test inputs
would notice it:
  "swap12"     corners 1 and 2 exchange their cells (the basis weights stay)
  "clamp"      the cell wrap (f + 1) % 5 replaced by min(f + 1, 4)
  "empty_neginf"  a destination without in-edges takes max = -inf instead of 0
  "empty_root" a destination without in-edges gets its root product alone (no bias)
  "drop_last"  the last in-edge (CSR order) of every destination is left out
"""
import numpy as np

NCELL = 26          # 25 spline cells + the root weight as cell 25
D = 768


def bf16_round(a):
    """float32 -> the nearest bfloat16 (ties to even), returned as float32.  Finite inputs."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def ref_plan(src, dst, pseudo, num_nodes, nmax, variant=None):
    """The plan of one side-batch.  src / dst: global node ids b * nmax + local; -> dict of
    g (E,), cells (E, 4), basis (E, 4) float32, mask (num_nodes,), cell_off (27,), arows, rowid
    (num_nodes, 26; -1 where the node has no row in the cell), dst_ptr (num_nodes + 1,), csr_e (E,),
    nbr_local (E,), src4 / cell4 (E, 4) (per CSR slot: source node and cell of each corner), rows4
    (E, 4) and basis4 (E, 4) float32 (per CSR slot)."""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    E = src.shape[0]
    p = np.asarray(pseudo, dtype=np.float32).reshape(E, 2)
    v = p * np.float32(4.0)
    fl = np.floor(v)
    fr = (v - fl).astype(np.float32)
    f = fl.astype(np.int64)
    g = f[:, 0] + 5 * f[:, 1]
    one = np.float32(1.0)
    cells = np.zeros((E, 4), dtype=np.int64)
    basis = np.zeros((E, 4), dtype=np.float32)
    for s in range(4):
        k0, k1 = s & 1, s >> 1
        if variant == "clamp":
            c0, c1 = np.minimum(f[:, 0] + k0, 4), np.minimum(f[:, 1] + k1, 4)
        else:
            c0, c1 = (f[:, 0] + k0) % 5, (f[:, 1] + k1) % 5
        cells[:, s] = c0 + 5 * c1
        b = one * (fr[:, 0] if k0 else one - fr[:, 0])
        b = b.astype(np.float32) * (fr[:, 1] if k1 else one - fr[:, 1])
        basis[:, s] = b.astype(np.float32)
    if variant == "swap12":
        cells = cells[:, [0, 2, 1, 3]]
    mask = np.full(num_nodes, 1 << 25, dtype=np.int64)
    for s in range(4):
        np.bitwise_or.at(mask, src, np.left_shift(1, cells[:, s]))
    cell_off = np.zeros(NCELL + 1, dtype=np.int64)
    rowid = np.full((num_nodes, NCELL), -1, dtype=np.int64)
    arows = []
    for k in range(NCELL):
        nodes = np.nonzero((mask >> k) & 1)[0]                # ascending node order
        rowid[nodes, k] = cell_off[k] + np.arange(nodes.size)
        arows.append(nodes)
        cell_off[k + 1] = cell_off[k] + nodes.size
    arows = np.concatenate(arows)
    dst_ptr = np.zeros(num_nodes + 1, dtype=np.int64)
    np.cumsum(np.bincount(dst, minlength=num_nodes), out=dst_ptr[1:])
    local = src % nmax
    csr_e = np.lexsort((np.arange(E), local, dst))            # by dst, then local source, then edge id
    src4 = np.repeat(src[csr_e][:, None], 4, axis=1)
    cell4 = cells[csr_e]
    return dict(E=E, num_nodes=num_nodes, nmax=nmax, g=g, cells=cells, basis=basis, mask=mask, cell_off=cell_off,
                arows=arows, rowid=rowid, dst_ptr=dst_ptr, csr_e=csr_e, nbr_local=local[csr_e], src4=src4,
                cell4=cell4, rows4=rowid[src4, cell4], basis4=basis[csr_e])


def ref_products(x, plan, W, dtype="f32"):
    """Product rows in float64: row r of cell k is x[arows[r]] @ W[k]^T (W: (26, 768 out, 768 in),
    cell 25 = the root weight).  dtype "bf16": x and W rounded to bfloat16 first, as the bf16
    kernel's operands are."""
    x, W = np.asarray(x), np.asarray(W)
    if dtype == "bf16":
        x, W = bf16_round(x.astype(np.float32)), bf16_round(W.astype(np.float32))
    x, off = x.astype(np.float64), plan["cell_off"]
    Y = np.zeros((int(off[NCELL]), W.shape[1]), dtype=np.float64)
    for k in range(NCELL):
        if off[k + 1] > off[k]:
            Y[off[k]:off[k + 1]] = x[plan["arows"][off[k]:off[k + 1]]] @ W[k].astype(np.float64).T
    return Y


def ref_messages(Y, plan):
    """Per CSR slot: (message, sum_s |b_s y_s|), the 4 corners added in the order s = 0..3."""
    r4, b4 = plan["rows4"], plan["basis4"].astype(np.float64)
    msg = np.zeros((plan["E"], Y.shape[1]), dtype=np.float64)
    mag = np.zeros_like(msg)
    for s in range(4):
        t = b4[:, s:s + 1] * Y[r4[:, s]]
        msg += t
        mag += np.abs(t)
    return msg, mag


def ref_combine(Y, plan, bias, mode, xres=None, nvalid=None, variant=None):
    """The layer from its product rows Y (float64): per destination the max of its in-edges'
    messages (0 without in-edges), + root row + bias; mode 0: ReLU, mode 1: xres + 0.1 * (.);
    rows of padded nodes (local index >= nvalid[graph]) are 0.  -> (out, S) with
    S = max_e sum_s |b_s y_s| + |root| + |bias| + |xres|, the magnitude every fp32 partial sum of
    the kernel is bounded by."""
    N, nmax, ptr = plan["num_nodes"], plan["nmax"], plan["dst_ptr"]
    msg, mag = ref_messages(Y, plan)
    C = Y.shape[1]
    m = np.zeros((N, C), dtype=np.float64)
    ms = np.zeros((N, C), dtype=np.float64)
    for vtx in range(N):
        a, b = int(ptr[vtx]), int(ptr[vtx + 1])
        if variant == "drop_last" and b > a:
            b -= 1
        if b > a:
            m[vtx] = msg[a:b].max(axis=0)
            ms[vtx] = mag[a:b].max(axis=0)
        elif variant == "empty_neginf":
            m[vtx] = -np.inf
    root = Y[plan["cell_off"][25] + np.arange(N)]
    bias = np.asarray(bias, dtype=np.float64)
    o = (m + root) + bias
    if variant == "empty_root":
        empty = np.diff(ptr) == 0
        o[empty] = root[empty]
    S = ms + np.abs(root) + np.abs(bias)
    if mode & 1:
        xr = np.asarray(xres, dtype=np.float64)
        out = xr + 0.1 * o
        S = S + np.abs(xr)
    else:
        out = np.maximum(o, 0.0)
    if nvalid is not None:
        pad = (np.arange(N) % nmax) >= np.repeat(np.asarray(nvalid, dtype=np.int64), nmax)[:N]
        out[pad] = 0.0
    return out, S


def ref_layer(x, plan, W, bias, mode, xres=None, nvalid=None, dtype="f32", variant=None):
    """One SplineConv layer in float64 from the definition -> (out, S)."""
    return ref_combine(ref_products(x, plan, W, dtype), plan, bias, mode, xres, nvalid, variant)


U_BF16 = 2.0 ** -8      # bfloat16 unit roundoff (8 significant bits, round to nearest)


def bf16_layer_bound(x, dx, plan, W, Y):
    """Worst-case bound of what the bf16 operand mode changes in one layer's pre-activation, given
    the fp32 layer (input x, product rows Y) and a bound dx of the input's own deviation: x and W
    rounded to bfloat16 (relative U_BF16 each), the product rows stored as bfloat16, propagated
    through the messages (basis weights >= 0), the max (1-Lipschitz) and the root add."""
    ax, aW = np.abs(np.asarray(x, dtype=np.float64)), np.abs(np.asarray(W, dtype=np.float64))
    dxr = dx + U_BF16 * (ax + dx)                                 # deviation of the rounded operand rows
    a1 = ref_products(dxr, plan, aW)                              # |dx~| |W|^T
    a2 = ref_products(ax + dxr, plan, aW)                         # |x~| |W|^T, times U for the rounded W
    dY = a1 + U_BF16 * a2
    dY = dY + U_BF16 * (np.abs(Y) + dY)                           # the stored row
    dmsg, _ = ref_messages(dY, plan)
    N, ptr = plan["num_nodes"], plan["dst_ptr"]
    do = dY[plan["cell_off"][25] + np.arange(N)].copy()
    for vtx in range(N):
        a, b = int(ptr[vtx]), int(ptr[vtx + 1])
        if b > a:
            do[vtx] += dmsg[a:b].max(axis=0)
    return do


def bf16_sconv_bound(x, plan, W0, b0, W1, b1, nvalid=None):
    """Elementwise bound of |bf16-mode output - fp32-mode output| of both layers chained (the bf16
    mode stores h as bfloat16; its final fp32 rows are not rounded)."""
    Y0 = ref_products(x, plan, W0)
    h, _ = ref_combine(Y0, plan, b0, 0, None, nvalid)
    dh = bf16_layer_bound(x, np.zeros_like(h), plan, W0, Y0)      # ReLU is 1-Lipschitz
    dh = dh + U_BF16 * (np.abs(h) + dh)                           # h stored as bfloat16
    Y1 = ref_products(h, plan, W1)
    return 0.1 * bf16_layer_bound(h, dh, plan, W1, Y1)


def ref_sconv(x, plan, W0, b0, W1, b1, nvalid=None, dtype="f32", variant=None):
    """Both layers chained (SiameseSConvOnNodes): h = layer 0 in mode 0, out = x + 0.1 * layer 1(h).
    dtype "bf16": h is rounded to bfloat16 between the layers (the kernel stores it so)."""
    h, _ = ref_layer(x, plan, W0, b0, 0, None, nvalid, dtype, variant)
    if dtype == "bf16":
        h = bf16_round(h.astype(np.float32))
    return ref_layer(h, plan, W1, b1, 1, x, nvalid, dtype, variant)
