"""Thin torch-tensor wrappers over the C-ABI (``include/fpm.h``).

Every op takes device tensors, checks shapes/dtypes on the host, and launches on the current
torch stream.  Outputs are caller-allocated (``torch.empty`` on the tensor's device).  There is
no CPU fallback: a CPU tensor or a missing library raises (``rank_topk``, ``rank_select``, ``rank_keep``,
``mate_rank``, ``score_census``, ``score_select``, ``rows_pool``, ``desc_score``, ``topk_merge``,
``group_scores``, ``group_topr``, ``cohort_decide``, ``coarse_score`` / ``coarse_pairs``, ``rows_fetch``,
``rows_pack``, ``rows_move`` and ``rows_quant8`` alone keep a plain-torch host path for CPU tensors: the statements
of the ordering and of the merge of
sorted lists, of the group fusions, of the cohort statistics, of the coarse score and of the ragged copies, which the
tests hold the kernels to).
"""
import ctypes

import torch

from . import _lib

F32, BF16 = 0, 1
EPI_STORE, EPI_RELU, EPI_TANH, EPI_AFFINITY, EPI_HALF_AFFINITY = 0, 1, 2, 3, 4
EPI_NORM_OUT = 6


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream(t=None):
    dev = t.device if t is not None else torch.device("cuda")
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.FpmError("fpm op called with a CPU tensor: the HIP path has no CPU fallback")


def _shape(t, shape, what):
    """Host-side operand check before a launch: ``t`` must cover ``shape`` exactly."""
    if t is not None and tuple(t.shape) != tuple(int(x) for x in shape):
        raise _lib.FpmError("%s: tensor of shape %s where %s is required" % (what, tuple(t.shape), tuple(shape)))


def _code(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise _lib.FpmError("unsupported operand dtype %s" % t.dtype)


def sinkhorn(s, n1, n2, iters, tau, dummy_row=True, out=None, n1max=None, n2max=None):
    """pygm-style log Sinkhorn on the (n1max, n2max) box of each pair.  ``s`` may be any strided
    3-D view (B, n1max, n2max); ``out`` likewise (allocated contiguous if None)."""
    _dev(s, n1, n2)
    B = s.shape[0]
    n1max = n1max or s.shape[1]
    n2max = n2max or s.shape[2]
    if out is None:
        out = torch.empty(B, n1max, n2max, device=s.device, dtype=torch.float32)
    _shape(out, (B, n1max, n2max), "sinkhorn out")
    _shape(n1, (B,), "sinkhorn n1")
    _shape(n2, (B,), "sinkhorn n2")
    # boxes over 256: the streaming kernel's split form needs a workspace of its own per call (exchange
    # slots + arrival counters; allocated on the caller's stream, so concurrent streams never share one)
    wsb = int(_lib.load().fpm_sinkhorn_ws_bytes(B, n1max, n2max)) if max(n1max, n2max) > 256 else 0
    ws = torch.empty(wsb, device=s.device, dtype=torch.uint8) if wsb > 0 else None
    _lib.call("fpm_sinkhorn_log_fwd_ws", _p(s), s.stride(0), s.stride(1), s.stride(2), _p(out), out.stride(0),
              out.stride(1), out.stride(2), _p(n1), _p(n2), B, n1max, n2max, int(iters), float(tau),
              int(bool(dummy_row)), _p(ws), wsb, _stream(s))
    return out


def soft_topk_fwd(ss, n1, n2, k, iters=10, tau=0.01, out=None, steps=None, out_host=None):
    """``out_host``: optional pinned host tensor written by the kernel as well (zero-copy D2H of
    ds_mat for the host Hungarian)."""
    _dev(ss, n1, n2, k)
    B, n1max, n2max = ss.shape
    if out is None:
        out = torch.empty(B, n1max, n2max, device=ss.device, dtype=torch.float32)
    _shape(out, (B, n1max, n2max), "soft_topk out")
    for t, w in ((n1, "n1"), (n2, "n2"), (k, "k"), (steps, "steps")):
        _shape(t, (B,), "soft_topk " + w)
    if out_host is not None and (out_host.is_cuda or not out_host.is_pinned() or tuple(out_host.shape) != (B, n1max, n2max)):
        raise _lib.FpmError("soft_topk: out_host must be a pinned host tensor of shape (B, n1max, n2max)")
    _lib.call("fpm_soft_topk_fwd", _p(ss), ss.stride(0), ss.stride(1), _p(n1), _p(n2), _p(k), B, n1max, n2max,
              int(iters), float(tau), _p(out), out.stride(0), out.stride(1), _p(steps), _p(out_host),
              out_host.stride(0) if out_host is not None else 0, out_host.stride(1) if out_host is not None else 0,
              _stream(ss))
    return out


def topk_select(ds, assign, k, lsa_out=None, out=None):
    _dev(ds, assign, k)
    B, n1max, n2max = ds.shape
    _shape(assign, (B, n1max), "topk_select assign")
    _shape(k, (B,), "topk_select k")
    _shape(out, (B, n1max, n2max), "topk_select out")
    _shape(lsa_out, (B, n1max, n2max), "topk_select lsa_out")
    perm = out if out is not None else torch.empty(B, n1max, n2max, device=ds.device, dtype=torch.float32)
    _lib.call("fpm_topk_select", _p(ds), ds.stride(0), ds.stride(1), _p(assign), assign.stride(0), _p(k), B,
              n1max, n2max, _p(perm), perm.stride(0), perm.stride(1), _p(lsa_out),
              lsa_out.stride(0) if lsa_out is not None else 0, lsa_out.stride(1) if lsa_out is not None else 0,
              _stream(ds))
    return perm


def profiling():
    """True while the library's HIP-event profiling of the product GEMM is on (fpm_profile_enable)."""
    return bool(_lib.load().fpm_profile_enabled())


_TUNING_GEN = [0]


def set_tuning(key, value):
    """Kernel-variant switch (fpm_set_tuning, include/fpm.h lists the keys).  Returns the previous
    value.  Every call bumps ``tuning_generation()`` (captured HIP graphs bake the variant in)."""
    prev = int(_lib.load().fpm_set_tuning(key.encode(), int(value)))
    if prev < 0:
        raise _lib.FpmError(_lib.load().fpm_last_error().decode(errors="replace"))
    _TUNING_GEN[0] += 1
    if key in WRONG_RESULT_PROBES:
        if int(value):
            _PROBES_ON.add(key)
        else:
            _PROBES_ON.discard(key)
    return prev


# timing probes whose results are wrong (gated by FPM_TIMING_PROBES=1 in the library); Net.run
# refuses to produce outputs while one of them is on
WRONG_RESULT_PROBES = ("gnn_mlp_off",)
_PROBES_ON = set()


def timing_probes_on():
    """Wrong-result timing probes currently switched on through ``set_tuning``."""
    return sorted(_PROBES_ON)


def tuning_generation():
    """Number of ``set_tuning`` calls so far (part of Net's graph-cache key)."""
    return _TUNING_GEN[0]


def gemm(A, B, M, N, K, lda, ldb, batch=1, sA=0, sB=0, a_rows=None, epi=EPI_STORE, bias=None, out_f=None,
         out_t=None, ldc=None, sC=0, n1=None, n2=None):
    """C = epi(A @ B^T (+bias)); A: rows of length >= K (lda), B: N x K (ldb)."""
    _dev(A, B)
    code = _code(A)
    if _code(B) != code:
        raise _lib.FpmError("gemm: A and B dtypes differ")
    if out_t is not None and _code(out_t) != code:
        raise _lib.FpmError("gemm: out_t dtype must match operands")
    _lib.call("fpm_gemm", code, _p(A), lda, sA, _p(a_rows), _p(B), ldb, sB, int(M), int(N), int(K), int(batch),
              int(epi), _p(bias), _p(out_f), _p(out_t), ldc if ldc is not None else N, sC, _p(n1), _p(n2),
              _stream(A))


def coef_tanh(g, wT, bias, out):
    """out[b] = tanh(g[b] @ wT + bias): g (B, K) fp32 rows, wT (K, N) fp32 -> out (B, N) (fpm_coef_tanh)."""
    _dev(g, wT, bias, out)
    B, K = g.shape
    N = wT.shape[1]
    if wT.shape[0] != K or g.stride(1) != 1 or not wT.is_contiguous() or tuple(out.shape) != (B, N):
        raise _lib.FpmError("coef_tanh: shapes g (B, K), wT (K, N) contiguous, out (B, N) expected")
    _lib.call("fpm_coef_tanh", _p(g), g.stride(0), _p(wT), _p(bias), B, K, N, _p(out), out.stride(0), _stream(g))
    return out


def global_weights(w1, w2, out=None):
    """normalize_over_channels(cat(w1, w2)) per pair (ngm.py:262-268) -> (B, D1 + D2) fp32."""
    _dev(w1, w2)
    if w1.dtype != torch.float32 or w2.dtype != torch.float32 or w1.stride(1) != 1 or w2.stride(1) != 1:
        raise _lib.FpmError("global_weights: float32 rows with unit stride expected")
    B, D1 = w1.shape
    D2 = w2.shape[1]
    _shape(w2, (B, D2), "global_weights w2")
    if out is None:
        out = torch.empty(B, D1 + D2, device=w1.device, dtype=torch.float32)
    _shape(out, (B, D1 + D2), "global_weights out")
    _lib.call("fpm_global_weights", _p(w1), w1.stride(0), _p(w2), w2.stride(0), B, D1, D2, _p(out), out.stride(0),
              _stream(w1))
    return out


def split_bf16x3(x, Kp, out=None):
    """(rows, K) fp32 rows -> (rows, 3 * Kp) bf16 [hi | lo | hi] split operands (fpm_split_bf16x3)."""
    _dev(x)
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
        raise _lib.FpmError("split_bf16x3: (rows, K) float32 rows with unit stride expected")
    rows, K = x.shape
    if out is None:
        out = torch.empty(rows, 3 * Kp, device=x.device, dtype=torch.bfloat16)
    _shape(out, (rows, 3 * Kp), "split_bf16x3 out")
    _lib.call("fpm_split_bf16x3", _p(x), x.stride(0), rows, K, int(Kp), _p(out), out.stride(0), _stream(x))
    return out


def split_weights_bf16x3(W, Kp):
    """(N, K) fp32 weights -> (N, 3 * Kp) bf16 [W_hi | W_hi | W_lo] (parameter packing, host side)."""
    N, K = W.shape
    Wp = torch.nn.functional.pad(W.float(), (0, Kp - K))
    hi = Wp.to(torch.bfloat16)
    lo = (Wp - hi.float()).to(torch.bfloat16)
    return torch.cat([hi, hi, lo], dim=1).contiguous()


def cast_bf16(x, out=None):
    _dev(x)
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    _lib.call("fpm_cast_bf16", _p(x), _p(out), x.numel(), _stream(x))
    return out


def spline_plan(src, dst, pseudo, num_nodes, nmax, max_graph_edges=0):
    """``max_graph_edges``: the largest per-graph edge count (host-known, e.g. from the batch's edge
    offsets) -> the per-graph plan kernels when it allows; 0 -> the global plan kernels.
    Edges are grouped by graph, in graph order; inside a graph any order gives the same plan."""
    _dev(src, dst, pseudo)
    E = src.numel()
    nbytes = _lib.load().fpm_spline_plan_bytes(E, num_nodes)
    ws = torch.empty(nbytes, device=src.device, dtype=torch.uint8)
    _lib.call("fpm_spline_plan_graphs", _p(src), _p(dst), _p(pseudo), E, num_nodes, nmax, int(max_graph_edges), _p(ws),
              nbytes, _stream(src))
    return ws


def spline_plan_jobs(parts, side, nmax):
    """The device job table of spline_plans_multi for ``parts`` (built once, cached while the first
    part lives; its host-to-device copy must not run inside a graph capture) -> tuple or None."""
    first = parts[0]
    dev = first.src[side].device
    key = (id(first), len(parts), side)
    store = _PLAN_JOBS.get(key)
    if store is not None and store[0]() is first:
        return store
    import weakref
    jobs, off, gstart = [], 0, 0
    for p in parts:
        E, nn = p.E[side], p.B * nmax
        if not (0 < p.max_graph_edges(side) <= 4096 and 26 <= nmax <= 1024 and p.B + 1 <= E):
            _PLAN_JOBS[key] = store = (weakref.ref(first), None)
            return store
        nbytes = int(_lib.load().fpm_spline_plan_bytes(E, nn))
        jobs.append([p.src[side].data_ptr(), p.dst[side].data_ptr(), p.pseudo[side].data_ptr(), E, nn, off,
                     (gstart << 32) | p.B])
        off += (nbytes + 255) // 256 * 256
        gstart += p.B
    if int(_lib.load().fpm_spline_plan_job_bytes()) != 56:
        raise _lib.FpmError("spline_plans_multi: PlanJob layout mismatch")
    table = torch.tensor(jobs, dtype=torch.int64).to(dev)
    sizes = [int(_lib.load().fpm_spline_plan_bytes(p.E[side], p.B * nmax)) for p in parts]
    store = (weakref.ref(first), table, [j[5] for j in jobs], sizes, off, gstart)
    _PLAN_JOBS[key] = store
    if len(_PLAN_JOBS) > 64:
        for k in [k for k, v in _PLAN_JOBS.items() if v[0]() is None]:
            del _PLAN_JOBS[k]
    return store


def spline_plans_multi(parts, side, nmax):
    """The spline plans of ``side`` for every sub-batch in ``parts`` (pipeline chunks of one batch)
    by one launch of each per-graph plan kernel (fpm_spline_plan_multi) -> list of plan workspaces
    (views into one allocation), each identical to spline_plan() of that sub-batch alone; None when
    some sub-batch needs the global plan kernels (graphs over 4096 edges, nmax outside [26, 1024])."""
    store = spline_plan_jobs(parts, side, nmax)
    if store[1] is None:
        return None
    _, table, offs, sizes, total, ngraphs = store
    ws = torch.empty(total, device=table.device, dtype=torch.uint8)
    _lib.call("fpm_spline_plan_multi", _p(table), len(parts), ngraphs, nmax, _p(ws), _stream(ws))
    return [ws[o:o + n] for o, n in zip(offs, sizes)]


_PLAN_JOBS = {}


def plan_csr(ws, E, num_nodes):
    """(dst_ptr, nbr_local) raw device pointers (ints) inside a plan workspace."""
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.call("fpm_spline_plan_csr", _p(ws), E, num_nodes, ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def spline_y_ws(dtype_code, E, num_nodes, device):
    """Product-row scratch for spline_conv (shared by both layers of a side)."""
    nbytes = _lib.load().fpm_spline_y_bytes(dtype_code, E, num_nodes)
    return torch.empty(nbytes, device=device, dtype=torch.uint8)


def spline_conv(x_op, plan, E, num_nodes, nmax, nvalid, W, bias, y_ws, mode, xres=None, cscale=None, out_f=None,
                out_t=None, argmax=None):
    """W: (26, 768, 768) = spline cells [cell][out][in] then root^T.  argmax (num_nodes, 768) int32:
    optional per-channel max in-edge slots for spline_conv_bwd_data(..., rplan=, argmax=)."""
    _dev(x_op, plan, W, bias, y_ws)
    code = _code(x_op)
    if _code(W) != code or tuple(W.shape) != (26, 768, 768):
        raise _lib.FpmError("spline_conv: W must be (26, 768, 768) in the operand dtype")
    if argmax is not None:
        _shape(argmax, (num_nodes, 768), "spline_conv argmax")
        if argmax.dtype != torch.int32:
            raise _lib.FpmError("spline_conv: argmax must be int32")
        _lib.call("fpm_spline_conv_fwd_argmax", code, _p(x_op), _p(plan), E, num_nodes, nmax, _p(nvalid), _p(W),
                  _p(bias), _p(y_ws), y_ws.numel(), int(mode), _p(xres), _p(cscale), _p(out_f), _p(out_t),
                  _p(argmax), _stream(x_op))
        return
    _lib.call("fpm_spline_conv_fwd", code, _p(x_op), _p(plan), E, num_nodes, nmax, _p(nvalid), _p(W), _p(bias),
              _p(y_ws), y_ws.numel(), int(mode), _p(xres), _p(cscale), _p(out_f), _p(out_t), _stream(x_op))


def rows_bcast_scale(y, B, coef=None, out_f=None, out_t=None, split=0):
    """Shared-graph SplineConv output y (rows, 768) fp32 -> B pairs (out_f copies, out_t scaled by coef[b]);
    ``split`` 1 / 2: bf16 out_t rows of 2304 columns [hi | lo | hi] / [hi | hi | lo] (spline_conv's mode >> 1)."""
    _dev(y, coef, out_f, out_t)
    code = _code(out_t) if out_t is not None else F32
    _lib.call("fpm_rows_bcast_scale", code, _p(y), y.shape[0], int(B), _p(coef), _p(out_f), _p(out_t), int(split),
              _stream(y))


def rows_gather_scale(y, row_off, idx, nmax, coef=None, out_f=None, out_t=None, split=0, idx_host=None,
                      row_off_host=None):
    """Cached SplineConv rows of an enrolled gallery -> a batch's padded operand rows
    (fpm_rows_gather_scale): y (sum n_g, 768) fp32, graph g at rows [row_off[g], row_off[g + 1])
    (row_off int64 [G + 1]); pair b takes graph idx[b] (int32 [B]) into rows [b * nmax, (b + 1) * nmax)
    of out_f (fp32 copies) and out_t (scaled by coef[b]; ``split`` as rows_bcast_scale), zeros past n_g.

    Checked on the host before anything is launched: dtype, contiguity and device of idx / row_off,
    every idx value in [0, G), every selected n_g <= nmax.  ``idx_host`` / ``row_off_host``: host
    copies of the two (a caller that built them on the host passes them, and the check needs no
    device synchronisation; without them the device tensors are copied back)."""
    for name, t, dt in (("idx", idx, torch.int32), ("row_off", row_off, torch.int64)):
        _check_index_tensors("rows_gather_scale", ((name, t, dt),))
        _check_on_device_of("rows_gather_scale", y, ((name, t),))
    _check_row_store("rows_gather_scale", "y", y)
    G, B, nmax = int(row_off.numel()) - 1, int(idx.numel()), int(nmax)
    if G < 1 or nmax < 0:
        raise _lib.FpmError("rows_gather_scale: empty gallery or negative nmax")
    ih, oh = _check_selection("rows_gather_scale", idx, row_off, y, "y", idx_host, row_off_host)
    if B and int((oh[ih + 1] - oh[ih]).max()) > nmax:
        raise _lib.FpmError("rows_gather_scale: a selected graph has n_g = %d > nmax = %d"
                            % (int((oh[ih + 1] - oh[ih]).max()), nmax))
    if split not in (0, 1, 2):
        raise _lib.FpmError("rows_gather_scale: split must be 0, 1 or 2")
    _shape(coef, (B, 768), "rows_gather_scale coef")
    _shape(out_f, (B * nmax, 768), "rows_gather_scale out_f")
    _shape(out_t, (B * nmax, 2304 if split else 768), "rows_gather_scale out_t")
    for t in (coef, out_f):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise _lib.FpmError("rows_gather_scale: coef / out_f must be contiguous fp32")
    if out_t is not None and not out_t.is_contiguous():
        raise _lib.FpmError("rows_gather_scale: out_t must be contiguous")
    _dev(y, row_off, idx, coef, out_f, out_t)
    code = _code(out_t) if out_t is not None else F32
    if split and code != BF16:
        raise _lib.FpmError("rows_gather_scale: split rows need a bf16 out_t")
    _lib.call("fpm_rows_gather_scale", code, _p(y), _p(row_off), _p(idx), G, B, nmax, _p(coef), _p(out_f), _p(out_t),
              int(split), _stream(y))


def rows_fetch(src, row_off, idx, out, out_off, idx_host=None, row_off_host=None, out_off_host=None):
    """Ragged row copy (fpm_rows_fetch): the rows of the entries idx[m] (int32 [M]) of ``src``
    ((sum n_g, 768) fp32, graph g at rows [row_off[g], row_off[g + 1]), row_off int64 [G + 1]) packed
    into ``out`` ((>= sum of the selected n_g, 768) fp32), entry m at rows [out_off[m], out_off[m + 1])
    (out_off int64 [M + 1], rising from 0 by the selected n_g) -> out.

    ``src`` is a device tensor, or a pinned host tensor, which the kernel reads through its device
    mapping (the rows of a shortlist out of an index whose fp32 rows live on the host); row_off, idx,
    out and out_off live on one device.  Checked on the host before anything is launched: dtypes,
    contiguity, devices, every idx in [0, G), the offsets, ``out`` large enough (``idx_host`` /
    ``row_off_host`` / ``out_off_host``: host copies, so the check needs no device synchronisation;
    without them the device tensors are copied back).  All-CPU tensors take the torch statement of
    the copy."""
    _check_index_tensors("rows_fetch", (("idx", idx, torch.int32), ("row_off", row_off, torch.int64),
                                        ("out_off", out_off, torch.int64)))
    _check_row_store("rows_fetch", "src", src)
    _check_row_store("rows_fetch", "out", out)
    for name, t in (("row_off", row_off), ("idx", idx), ("out_off", out_off)):
        if t.device != out.device:
            raise _lib.FpmError("rows_fetch: %s is on %s, out on %s" % (name, t.device, out.device))
    if src.device != out.device and not (out.is_cuda and not src.is_cuda and src.is_pinned()):
        raise _lib.FpmError("rows_fetch: src is on %s, out on %s (a host src must be pinned)"
                            % (src.device, out.device))
    G, M = int(row_off.numel()) - 1, int(idx.numel())
    if G < 1:
        raise _lib.FpmError("rows_fetch: empty gallery")
    if out_off.numel() != M + 1:
        raise _lib.FpmError("rows_fetch: out_off must hold %d offsets (got %d)" % (M + 1, out_off.numel()))
    ih, oh = _check_selection("rows_fetch", idx, row_off, src, "src", idx_host, row_off_host)
    if M > 65535:
        raise _lib.FpmError("rows_fetch: at most 65535 entries per call")
    ng = oh[ih + 1] - oh[ih]
    total = int(ng.sum())
    if out.shape[0] < total:
        raise _lib.FpmError("rows_fetch: out holds %d rows, the selection has %d" % (out.shape[0], total))
    fh = _host_copy(out_off_host, out_off)
    if not torch.equal(fh, torch.cat([torch.zeros(1, dtype=torch.int64), ng.cumsum(0)])):
        raise _lib.FpmError("rows_fetch: out_off must rise from 0 by the selected entries' row counts")
    if not out.is_cuda:
        if M:
            out[:total] = torch.cat([src[int(oh[g]):int(oh[g + 1])] for g in ih.tolist()])
        return out
    if M and total:
        _lib.call("fpm_rows_fetch", _p(src), int(src.shape[0]), _p(row_off), _p(idx), G, M, int(ng.max()), _p(out),
                  int(out.shape[0]), _p(out_off), _stream(out))
    return out


def rows_pack(src, n, nmax, out_off, out32=None, out16=None, n_host=None, out_off_host=None):
    """Ragged row pack (fpm_rows_pack), the inverse of the padding: ``src`` ((B * nmax, 768) fp32 padded
    rows, graph b at rows [b * nmax, b * nmax + n[b]); n int32 [B]) packed into ``out32`` (fp32,
    unchanged) and / or ``out16`` (bf16, the bits of ``cast_bf16``), graph b at rows
    [out_off[b], out_off[b + 1]) of either (out_off int64 [B + 1], rising by n; it need not start at 0,
    so a sub-batch packs into its place in a whole index) -> (out32, out16).  One launch, one read of
    the source; padding rows are not read, rows outside the offsets are not written.

    Everything lives on one device.  Checked on the host before anything is launched: dtypes,
    contiguity, devices, 0 <= n[b] <= nmax, the offsets, both outputs large enough (``n_host`` /
    ``out_off_host``: host copies, so the check needs no device synchronisation; without them the
    device tensors are copied back).  All-CPU tensors take the torch statement of the copy and the
    rounding."""
    _check_index_tensors("rows_pack", (("n", n, torch.int32), ("out_off", out_off, torch.int64)))
    if out32 is None and out16 is None:
        raise _lib.FpmError("rows_pack: give out32, out16 or both")
    for name, t, dt in (("src", src, torch.float32), ("out32", out32, torch.float32), ("out16", out16, torch.bfloat16)):
        if t is not None or name == "src":
            _check_row_store("rows_pack", name, t, dt)
    for name, t in (("n", n), ("out_off", out_off), ("out32", out32), ("out16", out16)):
        if t is not None and t.device != src.device:
            raise _lib.FpmError("rows_pack: %s is on %s, src on %s" % (name, t.device, src.device))
    B, nmax = int(n.numel()), int(nmax)
    if nmax < 0:
        raise _lib.FpmError("rows_pack: negative nmax")
    if B > 65535:
        raise _lib.FpmError("rows_pack: at most 65535 graphs per call")
    if src.shape[0] != B * nmax:
        raise _lib.FpmError("rows_pack: src holds %d rows, %d graphs of nmax = %d have %d"
                            % (src.shape[0], B, nmax, B * nmax))
    if out_off.numel() != B + 1:
        raise _lib.FpmError("rows_pack: out_off must hold %d offsets (got %d)" % (B + 1, out_off.numel()))
    nh, oh = _host_copy(n_host, n), _host_copy(out_off_host, out_off)
    if nh.numel() != B or oh.numel() != B + 1:
        raise _lib.FpmError("rows_pack: host copies of n / out_off do not match the device tensors")
    if B and (int(nh.min()) < 0 or int(nh.max()) > nmax):
        raise _lib.FpmError("rows_pack: a graph has n = %d outside [0, nmax = %d]"
                            % (int(nh.max()) if int(nh.max()) > nmax else int(nh.min()), nmax))
    if int(oh[0]) < 0 or not torch.equal(oh[1:] - oh[:-1], nh):
        raise _lib.FpmError("rows_pack: out_off must rise from a non-negative offset by the graphs' row counts n")
    for name, t in (("out32", out32), ("out16", out16)):
        if t is not None and t.shape[0] < int(oh[-1]):
            raise _lib.FpmError("rows_pack: %s holds %d rows, the offsets end at %d" % (name, t.shape[0], int(oh[-1])))
    if not src.is_cuda:
        if B and int(nh.sum()):
            rows = torch.cat([src[b * nmax:b * nmax + k] for b, k in enumerate(nh.tolist())])
            if out32 is not None:
                out32[int(oh[0]):int(oh[-1])] = rows
            if out16 is not None:
                out16[int(oh[0]):int(oh[-1])] = rows.to(torch.bfloat16)
        return out32, out16
    if B and nmax and int(nh.sum()):
        out_rows = min(t.shape[0] for t in (out32, out16) if t is not None)
        _lib.call("fpm_rows_pack", _p(src), int(src.shape[0]), _p(n), B, nmax, _p(out_off), _p(out32), _p(out16),
                  int(out_rows), _stream(src))
    return out32, out16


def _ranges_meet(a0, a1, b0, b1):
    """Whether some range [a0[i], a1[i]) meets some range [b0[j], b1[j]) (host int64, none empty)."""
    if a0.numel() == 0 or b0.numel() == 0:
        return False
    order = torch.argsort(a0)
    start, reach = a0[order], torch.cummax(a1[order], 0)[0]
    # the ranges a that start before b's end: the furthest any of them reaches is past b's start
    before = torch.searchsorted(start, b1, right=False)
    return bool(((before > 0) & (reach[(before - 1).clamp(min=0)] > b0)).any())


def rows_move(src_off, dst_off, cnt, src32=None, dst32=None, src16=None, dst16=None, src_off_host=None,
              dst_off_host=None, cnt_host=None, src8=None, dst8=None, srcs=None, dsts=None):
    """Ragged segment copy (fpm_rows_move): segment k goes from rows [src_off[k], src_off[k] + cnt[k]) of the
    source to rows [dst_off[k], dst_off[k] + cnt[k]) of the destination (int64 [K] each, K <= 65535) -- the
    fp32 rows ``src32`` -> ``dst32``, the bf16 rows ``src16`` -> ``dst16`` (as bits: nothing is rounded), or
    both pairs from the one offset table, in one launch -> (dst32, dst16).  Rows outside the destination
    ranges are not written.  The rows of an fp8 index (fpm_rows_move8): ``src8`` -> ``dst8`` ((rows, 768)
    float8_e4m3fn, as bytes) with their scales ``srcs`` -> ``dsts`` ((rows,) fp32), all four and no other rows
    -> (dst8, dsts).

    Everything lives on one device.  Checked on the host before anything is launched: dtypes, contiguity,
    devices, every range inside its tensor, destination ranges that do not meet each other, and -- a pair's
    source and destination may be the same tensor, which is how an index is compacted inside its storage --
    that then no destination range meets a source range: the segments are copied in no particular order, so
    nothing that is read may be written.  A source and a destination that share memory without being the
    same rows are refused.  (``*_host``: host copies of the tables, so the check needs no device
    synchronisation; without them the device tensors are copied back.)  All-CPU tensors take the torch
    statement of the copy."""
    _check_index_tensors("rows_move", (("src_off", src_off, torch.int64), ("dst_off", dst_off, torch.int64),
                                       ("cnt", cnt, torch.int64)))
    if (src32 is None) != (dst32 is None) or (src16 is None) != (dst16 is None):
        raise _lib.FpmError("rows_move: src32 goes with dst32, src16 with dst16")
    fp8 = any(t is not None for t in (src8, dst8, srcs, dsts))
    if fp8 and (any(t is None for t in (src8, dst8, srcs, dsts)) or src32 is not None or src16 is not None):
        raise _lib.FpmError("rows_move: the fp8 rows go as src8, dst8, srcs and dsts together, without other rows")
    if src32 is None and src16 is None and not fp8:
        raise _lib.FpmError("rows_move: give the fp32 rows (src32, dst32), the bf16 rows (src16, dst16) or both")
    pairs = []
    for bits, s, d, dt in (("32", src32, dst32, torch.float32), ("16", src16, dst16, torch.bfloat16),
                           ("8", src8, dst8, torch.float8_e4m3fn)):
        if s is not None:
            _check_row_store("rows_move", "src" + bits, s, dt)
            _check_row_store("rows_move", "dst" + bits, d, dt)
            pairs.append((s, d, dt))
    if fp8:
        for name, t, rows in (("srcs", srcs, src8), ("dsts", dsts, dst8)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous() \
                    or t.numel() != rows.shape[0]:
                raise _lib.FpmError("rows_move: %s must be a contiguous fp32 tensor of one scale per row of its rows"
                                    % name)
        pairs.append((srcs, dsts, None))                     # the scales move with their rows: the same checks
    dev = pairs[0][1].device
    for name, t in (("src_off", src_off), ("dst_off", dst_off), ("cnt", cnt), ("src32", src32), ("dst32", dst32),
                    ("src16", src16), ("dst16", dst16), ("src8", src8), ("dst8", dst8), ("srcs", srcs),
                    ("dsts", dsts)):
        if t is not None and t.device != dev:
            raise _lib.FpmError("rows_move: %s is on %s, the destination on %s" % (name, t.device, dev))
    K = int(cnt.numel())
    if src_off.numel() != K or dst_off.numel() != K:
        raise _lib.FpmError("rows_move: %d source offsets, %d destination offsets and %d counts (one of each per "
                            "segment)" % (src_off.numel(), dst_off.numel(), K))
    if K > 65535:
        raise _lib.FpmError("rows_move: at most 65535 segments per call")
    sh, dh, ch = _host_copy(src_off_host, src_off), _host_copy(dst_off_host, dst_off), _host_copy(cnt_host, cnt)
    if sh.numel() != K or dh.numel() != K or ch.numel() != K:
        raise _lib.FpmError("rows_move: host copies of src_off / dst_off / cnt do not match the device tensors")
    src_rows = min(int(s.shape[0]) for s, _, _ in pairs)
    dst_rows = min(int(d.shape[0]) for _, d, _ in pairs)
    if K:
        if int(ch.min()) < 0:
            raise _lib.FpmError("rows_move: a negative row count (%d)" % int(ch.min()))
        if int(sh.min()) < 0 or int((sh + ch).max()) > src_rows:
            raise _lib.FpmError("rows_move: a source range outside the %d rows of the source" % src_rows)
        if int(dh.min()) < 0 or int((dh + ch).max()) > dst_rows:
            raise _lib.FpmError("rows_move: a destination range outside the %d rows of the destination" % dst_rows)
    some = ch > 0
    s0, d0, c = sh[some], dh[some], ch[some]
    order = torch.argsort(d0)
    if bool((d0[order][1:] < (d0 + c)[order][:-1]).any()):
        raise _lib.FpmError("rows_move: two destination ranges meet")
    for s, d, dt in pairs:
        lo_s, lo_d = s.data_ptr(), d.data_ptr()
        hi_s, hi_d = lo_s + s.numel() * s.element_size(), lo_d + d.numel() * d.element_size()
        if s.device != d.device or lo_s >= hi_d or lo_d >= hi_s:
            continue                                         # two buffers
        if lo_s != lo_d:
            raise _lib.FpmError("rows_move: the source and the destination share memory without being the same "
                                "rows; pass the one tensor as both")
        if _ranges_meet(s0, s0 + c, d0, d0 + c):
            raise _lib.FpmError("rows_move: source and destination are one tensor and a destination range meets a "
                                "source range (the segments are copied in no particular order; move such rows "
                                "through a staging buffer)")
    total = int(c.sum())
    if not dev.type == "cuda":
        if total:
            at = lambda o: torch.cat([torch.arange(a, a + k) for a, k in zip(o.tolist(), c.tolist())])
            rs, rd = at(s0), at(d0)
            for s, d, _ in pairs:
                d[rd] = s[rs]                                # the right side is gathered before anything is written
        return (dst8, dsts) if fp8 else (dst32, dst16)
    if fp8:
        if total:
            _lib.call("fpm_rows_move8", _p(src8), _p(srcs), src_rows, _p(src_off), _p(dst_off), _p(cnt), K,
                      int(c.max()), _p(dst8), _p(dsts), dst_rows, _stream(dst8))
        return dst8, dsts
    if total:
        _lib.call("fpm_rows_move", _p(src32), _p(src16), src_rows, _p(src_off), _p(dst_off), _p(cnt), K, int(c.max()),
                  _p(dst32), _p(dst16), dst_rows, _stream(pairs[0][1]))
    return dst32, dst16


QUANT8_MAX = 448.0             # the largest e4m3fn value
QUANT8_EMAX = 110              # |e| of a row scale 2^e at most: float(y8) * 2^e stays a normal bf16


def _quant8_host(y):
    """The definition of the fp8 row format in plain torch -> (y8 float8_e4m3fn, s8 fp32); see ``rows_quant8``."""
    amax = y.abs().amax(dim=1) if y.shape[0] else y.new_zeros(0)
    m, x = torch.frexp(amax)                                 # amax = m 2^x, 0.5 <= m < 1;  448 = 0.875 x 2^9
    e = torch.where(amax == 0, torch.zeros_like(x), x - 9 + (m > 0.875).to(x.dtype)).clamp(-QUANT8_EMAX, QUANT8_EMAX)
    one = torch.ones_like(amax)
    y8 = (y * torch.ldexp(one, -e)[:, None]).clamp(-QUANT8_MAX, QUANT8_MAX).to(torch.float8_e4m3fn)
    return y8, torch.ldexp(one, e)


def rows_dequant8(y8, s8):
    """The coarse operand of fp8 rows, (y8 * s8[:, None]) as bf16: exact (four significant bits, a power-of-two
    scale, a normal bf16 result), so no rounding happens here."""
    return (y8.to(torch.float32) * s8[:, None]).to(torch.bfloat16)


def rows_quant8(y, y8=None, s8=None):
    """Index rows to fp8 with a power-of-two scale per row (fpm_rows_quant8) -> (y8, s8): for a row of
    ``y`` ((rows, 768) fp32), amax = max |y[r]|; e = 0 if amax == 0, else with (m, x) = frexp(amax),
    e = x - 9 + (m > 0.875), the smallest e with amax <= 448 * 2^e, clamped to [-QUANT8_EMAX, QUANT8_EMAX];
    ``s8[r]`` = 2^e (fp32) and ``y8[r]`` = float8_e4m3fn(clamp(y[r] * 2^-e, -448, 448)), round to nearest even
    (the OCP encoding, torch's ``.to(torch.float8_e4m3fn)``).  The coarse operand of such a row,
    bf16(float(y8) * s8) (``rows_dequant8``), is exact.  Non-finite rows are the caller's error.

    Everything lives on one device.  Checked on the host before anything is launched: dtypes, contiguity,
    devices, sizes and 16-byte alignment.  ``rows`` = 0 launches nothing.  CPU tensors take the torch
    statement of the definition."""
    _check_row_store("rows_quant8", "y", y)
    rows = int(y.shape[0])
    if y8 is None:
        y8 = torch.empty(rows, 768, device=y.device, dtype=torch.float8_e4m3fn)
    if s8 is None:
        s8 = torch.empty(rows, device=y.device, dtype=torch.float32)
    if not isinstance(y8, torch.Tensor) or y8.dtype != torch.float8_e4m3fn or tuple(y8.shape) != (rows, 768) \
            or not y8.is_contiguous():
        raise _lib.FpmError("rows_quant8: y8 must be contiguous float8_e4m3fn rows of y's shape (%d, 768)" % rows)
    if not isinstance(s8, torch.Tensor) or s8.dtype != torch.float32 or tuple(s8.shape) != (rows,) \
            or not s8.is_contiguous():
        raise _lib.FpmError("rows_quant8: s8 must be a contiguous fp32 tensor of %d row scales" % rows)
    for name, t in (("y8", y8), ("s8", s8)):
        if t.device != y.device:
            raise _lib.FpmError("rows_quant8: %s is on %s, y on %s" % (name, t.device, y.device))
    if rows and (y.data_ptr() | y8.data_ptr()) & 15:
        raise _lib.FpmError("rows_quant8: y and y8 must be 16-byte aligned")
    if not y.is_cuda:
        q, sc = _quant8_host(y)
        y8.copy_(q)
        s8.copy_(sc)
        return y8, s8
    if rows:
        _lib.call("fpm_rows_quant8", _p(y), rows, _p(y8), _p(s8), _stream(y))
    return y8, s8


def rank_key(scores, ids=None):
    """The 64-bit ranking key (the host statement of csrc/rank_key.h) for a (P, G) fp32 tensor, as int64
    whose signed order is the key's unsigned order shifted by 2^63: (order-preserving bits of the score)
    << 32 | (0xFFFFFFFF - index); NaN maps below -inf, -0 below +0.  ``ids`` (integers of scores' shape,
    each in [0, 2^32)): taken in place of the column number (``topk_merge``'s key)."""
    s = scores.detach().to(torch.float32)
    u = s.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    neg = u >= 0x80000000
    bits = torch.where(neg, 0xFFFFFFFF - u, u + 0x80000000)
    bits = torch.where(torch.isnan(s), torch.zeros_like(bits), bits)
    if ids is None:
        i = torch.arange(s.shape[-1], device=s.device, dtype=torch.int64).expand_as(bits)
    else:
        i = ids.to(torch.int64) & 0xFFFFFFFF
    return ((bits - 0x80000000) << 32) | (0xFFFFFFFF - i)


def _top_outputs(op, scores, k, top_idx, top_score):
    """``rank_topk``'s and ``rank_select``'s outputs on the device path, the caller's or new ones."""
    _dev(top_idx, top_score)
    shape, msg = (int(scores.shape[0]), k), "top_idx must be contiguous int32, top_score contiguous fp32"
    return (_out_tensor(op, "top_idx", top_idx, shape, torch.int32, scores.device, msg),
            _out_tensor(op, "top_score", top_score, shape, torch.float32, scores.device, msg))


def rank_topk(scores, k, top_idx=None, top_score=None):
    """Per-row top-k of scores (P, G) fp32 (any row stride) -> (top_idx (P, k) int32, top_score (P, k)
    fp32): descending score, ties to the lower index, NaN after every number (NaNs by index).
    Device tensors run fpm_rank_topk; CPU tensors take the host path below (a stable sort on the same
    key), which states the semantics."""
    P, G = _check_scores("rank_topk", scores)
    k = int(k)
    if not 1 <= k <= min(G, 128):
        raise _lib.FpmError("rank_topk: k = %d outside [1, min(G, 128) = %d]" % (k, min(G, 128)))
    if not scores.is_cuda:
        order = _rank_order(scores, k)
        return order.to(torch.int32), torch.gather(scores, 1, order)
    scores, ld = _dense_rows(scores)
    top_idx, top_score = _top_outputs("rank_topk", scores, k, top_idx, top_score)
    _lib.call("fpm_rank_topk", _p(scores), ld, P, G, k, _p(top_idx), _p(top_score), _stream(scores))
    return top_idx, top_score


RANK_SELECT_KMAX = 1024


def rank_select(scores, k, top_idx=None, top_score=None):
    """``rank_topk``'s ranking for 1 <= k <= min(G, 1024) (the shortlist of a 1:N identification):
    scores (P, G) fp32 (any row stride) -> (top_idx (P, k) int32, top_score (P, k) fp32), descending,
    ties to the lower index, NaN after every number.  Device tensors run fpm_rank_select (a radix
    search for the k-th largest key over several workgroups per row, a compaction, a sort of the k in
    LDS); CPU tensors take the same stable sort as ``rank_topk``'s host path.  Keys are unique, so
    the two agree bit for bit, and with ``rank_topk`` for k <= 128."""
    P, G = _check_scores("rank_select", scores)
    k = int(k)
    if not 1 <= k <= min(G, RANK_SELECT_KMAX):
        raise _lib.FpmError("rank_select: k = %d outside [1, min(G, %d) = %d]"
                            % (k, RANK_SELECT_KMAX, min(G, RANK_SELECT_KMAX)))
    if not scores.is_cuda:
        order = _rank_order(scores, k)
        return order.to(torch.int32), torch.gather(scores, 1, order)
    if P > 65535:
        raise _lib.FpmError("rank_select: at most 65535 rows per call")
    scores, ld = _dense_rows(scores)
    top_idx, top_score = _top_outputs("rank_select", scores, k, top_idx, top_score)
    if P == 0:
        return top_idx, top_score
    ws, wsb = _scratch("fpm_rank_select_ws_bytes", scores.device, P)     # histograms, prefix states, the k keys
    _lib.call("fpm_rank_select", _p(scores), ld, P, G, k, _p(top_idx), _p(top_score), _p(ws), wsb, _stream(scores))
    return top_idx, top_score


def rank_keep(scores, k, keep=None):
    """The k best columns of every row as a set, in ascending column order, for any 1 <= k <= G (fpm_rank_keep;
    the prescreen of a 1:N identification): scores (P, G) fp32 (any row stride) -> keep (P, k) int32.  The
    ranking is ``rank_select``'s (``rank_key``: score descending, ties to the lower column, NaN after every
    number), so for k <= 1024 ``keep`` holds ``rank_select``'s indices, sorted.  Device tensors run the kernel
    (``rank_select``'s radix search for the k-th key, then an ordered compaction: counts per slice, their
    prefix, ballots; no atomics hand out a slot); CPU tensors take the statement: a stable descending sort on the
    key, the first k, sorted by column.  Keys are unique, so the two agree bit for bit."""
    P, G = _check_scores("rank_keep", scores)
    k = int(k)
    if not 1 <= k <= G:
        raise _lib.FpmError("rank_keep: k = %d outside [1, G = %d]" % (k, G))
    if P > 65535:
        raise _lib.FpmError("rank_keep: at most 65535 rows per call")
    keep = _out_tensor("rank_keep", "keep", keep, (P, k), torch.int32, scores.device,
                       "keep must be contiguous int32 on the scores' device")
    if not scores.is_cuda:
        return keep.copy_(torch.sort(_rank_order(scores, k), dim=1).values)
    if P == 0:
        return keep
    scores, ld = _dense_rows(scores)
    ws, wsb = _scratch("fpm_rank_keep_ws_bytes", scores.device, P, G)    # histograms, prefix states, slice counts
    _lib.call("fpm_rank_keep", _p(scores), ld, P, G, k, _p(keep), _p(ws), wsb, _stream(scores))
    return keep


# ---- evaluation of a search from its score matrices (``fpm.evaluate``) -----------------------------
CENSUS_TMAX = 4095
SCORE_CLASSES = ("genuine", "impostor")


def _eval_args(op, scores, row_lab, col_lab, own):
    """The common inputs of ``mate_rank``, ``score_census`` and ``score_select``, checked on the host before
    anything is launched -> (scores with dense columns, its row stride, P, G, the labels' leading dimension)."""
    P, G = _check_scores(op, scores)
    if G < 1:
        raise _lib.FpmError("%s: scores must have at least one column" % op)
    for name, t in (("row_lab", row_lab), ("col_lab", col_lab), ("own", own)):
        if t is None and name == "own":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or not t.is_contiguous():
            raise _lib.FpmError("%s: %s must be a contiguous int32 tensor (got %s)"
                                % (op, name, getattr(t, "dtype", type(t).__name__)))
        if t.device != scores.device:
            raise _lib.FpmError("%s: %s is on %s, scores on %s" % (op, name, t.device, scores.device))
    _shape(row_lab, (P,), "%s row_lab" % op)
    _shape(own, (P,), "%s own" % op)
    if tuple(col_lab.shape) not in ((G,), (P, G)):
        raise _lib.FpmError("%s: col_lab of shape %s where (G,) = %s or (P, G) = %s is required"
                            % (op, tuple(col_lab.shape), (G,), (P, G)))
    lab_ld = G if col_lab.dim() == 2 else 0
    scores, ld = _dense_rows(scores)
    return scores, ld, P, G, lab_ld


def score_classes(scores, row_lab, col_lab, own=None):
    """The classes of a score matrix, in plain torch -> (genuine, impostor) bool masks (P, G); a score in neither
    is ignored: a column with ``col_lab < 0``, and the column ``own[p]`` of row p.  Otherwise genuine where
    ``col_lab == row_lab[p]``, else impostor."""
    P, G = int(scores.shape[0]), int(scores.shape[1])
    cl = col_lab if col_lab.dim() == 2 else col_lab.view(1, G).expand(P, G)
    ign = cl < 0
    if own is not None:
        ign = ign | (torch.arange(G, device=scores.device, dtype=torch.int32).view(1, G) == own.view(P, 1))
    gen = ~ign & (cl == row_lab.view(P, 1))
    return gen, ~ign & ~gen


def mate_rank(scores, row_lab, col_lab, own=None):
    """Where every row's mate ranks among the impostors (fpm_mate_rank): scores (P, G) fp32 (any row stride),
    row_lab (P,) int32, col_lab (G,) or (P, G) int32, own (P,) int32 or None (``score_classes``) ->

        mate_col   (P,) int32  the genuine column with the greatest ``rank_key``, -1 if the row has none;
        mate_score (P,) fp32   that column's bits, NaN 0x7FC00000 if none;
        mate_rank  (P,) int32  the number of impostor columns whose key is above the mate's, -1 if none.

    The mate survives a cut to the K best exactly when ``mate_rank < K`` if the row has one genuine column; with
    several, the rank is the best one's and the other genuine columns also take places in the cut (each further
    impression needs the rank plus the genuine columns above it below K).  Device tensors
    run the kernels (a 64-bit integer atomic max, then integer adds); CPU tensors take the statement below.  Keys
    are unique and integer sums have one value, so the two agree bit for bit."""
    op = "mate_rank"
    scores, ld, P, G, lab_ld = _eval_args(op, scores, row_lab, col_lab, own)
    if not scores.is_cuda:
        gen, imp = score_classes(scores, row_lab, col_lab, own)
        key = rank_key(scores)
        low = torch.iinfo(torch.int64).min
        best = torch.where(gen, key, torch.full_like(key, low)).max(1).values if P else key.new_empty(0)
        has = gen.any(1)
        col = torch.where(has, 0xFFFFFFFF - (best & 0xFFFFFFFF), torch.full_like(best, -1))
        rank = (imp & (key > best.view(P, 1))).sum(1)
        qnan = torch.full((P,), 0x7FC00000, dtype=torch.int32).view(torch.float32)
        sc = torch.where(has, torch.gather(scores, 1, col.clamp(min=0).view(P, 1)).view(P).view(torch.int32),
                         qnan.view(torch.int32)).view(torch.float32)
        return col.to(torch.int32), sc, torch.where(has, rank, torch.full_like(rank, -1)).to(torch.int32)
    dev = scores.device
    mcol = torch.empty(P, device=dev, dtype=torch.int32)
    msc = torch.empty(P, device=dev, dtype=torch.float32)
    mrank = torch.empty(P, device=dev, dtype=torch.int32)
    if P == 0:
        return mcol, msc, mrank
    ws, wsb = _scratch("fpm_mate_rank_ws_bytes", dev, P)
    _lib.call("fpm_mate_rank", _p(scores), ld, P, G, _p(row_lab), _p(col_lab), lab_ld, _p(own), _p(mcol), _p(msc),
              _p(mrank), _p(ws), wsb, _stream(scores))
    return mcol, msc, mrank


def _check_edges(op, edges, scores):
    if not isinstance(edges, torch.Tensor) or edges.dtype != torch.float32 or edges.dim() != 1 \
            or not edges.is_contiguous():
        raise _lib.FpmError("%s: edges must be a contiguous 1-d fp32 tensor" % op)
    if edges.device != scores.device:
        raise _lib.FpmError("%s: edges is on %s, scores on %s" % (op, edges.device, scores.device))
    T = int(edges.numel())
    if not 1 <= T <= CENSUS_TMAX:
        raise _lib.FpmError("%s: T = %d edges outside [1, %d]" % (op, T, CENSUS_TMAX))
    eh = edges.cpu()
    if not bool(torch.isfinite(eh).all()):
        raise _lib.FpmError("%s: edges must be finite" % op)
    if T > 1 and not bool((eh[1:] > eh[:-1]).all()):
        raise _lib.FpmError("%s: edges must be strictly ascending" % op)
    return T


def score_census(scores, row_lab, col_lab, edges, own=None):
    """The histograms of the genuine and the impostor scores of a whole matrix (fpm_score_census): the common
    inputs of ``mate_rank``, and ``edges`` (T,) fp32, finite, strictly ascending, 1 <= T <= 4095 ->
    (gen (T + 1,) int64, imp (T + 1,) int64, skipped (3,) int64: NaN genuine, NaN impostor, ignored).
    bin(s) = the number of edges <= s (``torch.bucketize(s, edges, right=True)``): a score equal to an edge falls
    in the upper bin, -inf in bin 0, +inf in bin T.  gen.sum() + imp.sum() + skipped.sum() == P * G.  Device
    tensors run the kernel (32-bit histograms in LDS, 64-bit integer atomic adds), CPU tensors the statement;
    integer counts have one value, so the two agree exactly."""
    op = "score_census"
    scores, ld, P, G, lab_ld = _eval_args(op, scores, row_lab, col_lab, own)
    T = _check_edges(op, edges, scores)
    if not scores.is_cuda:
        gen, imp = score_classes(scores, row_lab, col_lab, own)
        nan = torch.isnan(scores)
        b = torch.bucketize(scores, edges, right=True)
        hist = lambda m: torch.bincount(b[m & ~nan].view(-1), minlength=T + 1)
        skipped = torch.stack([(gen & nan).sum(), (imp & nan).sum(), (~gen & ~imp).sum()])
        return hist(gen), hist(imp), skipped
    dev = scores.device
    out = torch.empty(2 * (T + 1) + 3, device=dev, dtype=torch.int64)
    gen, imp, skipped = out[:T + 1], out[T + 1:2 * T + 2], out[2 * T + 2:]
    _lib.call("fpm_score_census", _p(scores), ld, P, G, _p(row_lab), _p(col_lab), lab_ld, _p(own), _p(edges), T,
              _p(gen), _p(imp), _p(skipped), _stream(scores))
    return gen, imp, skipped


def score_select(scores, row_lab, col_lab, cls, k, own=None):
    """The k-th largest (1-based) non-NaN score of one class over a whole matrix (fpm_score_select): the common
    inputs of ``mate_rank``, ``cls`` "genuine" or "impostor", k >= 1 -> (value: a 0-d fp32 host tensor, the exact
    bits of that score -- -0 ranks below +0 --, NaN 0x7FC00000 when k exceeds the count; count: the class's number
    of non-NaN scores, an int).  Device tensors run three radix passes over the order-preserving score bits (11, 11
    and 10 bits), each histogram read back on the host (the call synchronises the stream: an offline tool); CPU
    tensors take a sort."""
    op = "score_select"
    scores, ld, P, G, lab_ld = _eval_args(op, scores, row_lab, col_lab, own)
    if cls not in SCORE_CLASSES:
        raise _lib.FpmError("%s: cls must be one of %s (got %r)" % (op, SCORE_CLASSES, cls))
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise _lib.FpmError("%s: k = %r must be an integer >= 1" % (op, k))
    if not scores.is_cuda:
        m = score_classes(scores, row_lab, col_lab, own)[SCORE_CLASSES.index(cls)] & ~torch.isnan(scores)
        n = int(m.sum())
        if k > n:
            return torch.full((), 0x7FC00000, dtype=torch.int32).view(torch.float32), n
        key = rank_key(scores[m].view(1, -1), ids=torch.zeros(1, n, dtype=torch.int64))[0]
        at = torch.argsort(key, descending=True, stable=True)[k - 1]
        return scores[m][at].clone(), n
    value, count = ctypes.c_float(), ctypes.c_long()
    ws, wsb = _scratch("fpm_score_select_ws_bytes", scores.device)
    _lib.call("fpm_score_select", _p(scores), ld, P, G, _p(row_lab), _p(col_lab), lab_ld, _p(own),
              1 + SCORE_CLASSES.index(cls), k, ctypes.byref(value), ctypes.byref(count), _p(ws), wsb, _stream(scores))
    bits = ctypes.c_int32.from_buffer_copy(value).value
    return torch.full((), bits, dtype=torch.int32).view(torch.float32), int(count.value)


DESC_DIM = 768
POOL_THREADS = 192             # rows_pool: a thread per four channels
POOL_TREE = 256                # rows_pool: the norm's tree runs over this many partial sums


def _rows_pool_host(y, off):
    """The definition of a template's descriptor in plain torch: y (R, 768) fp32, off (E + 1,) host int64 -> (E, 768)
    bf16; see ``rows_pool``."""
    E = int(off.numel()) - 1
    n = off[1:] - off[:-1]
    m = torch.zeros(E, DESC_DIM, dtype=torch.float32)
    zero = torch.zeros((), dtype=torch.float32)
    for i in range(int(n.max()) if E else 0):
        on = i < n                                               # a sum that started at +0.0 is never -0.0: + 0.0 is exact
        m = m + torch.where(on[:, None], y[torch.where(on, off[:-1] + i, torch.zeros_like(n))], zero)
    md = m.to(torch.float64)
    q = (md * md).view(E, POOL_THREADS, 4)
    p = torch.zeros(E, POOL_TREE, dtype=torch.float64)
    p[:, :POOL_THREADS] = ((q[:, :, 0] + q[:, :, 1]) + q[:, :, 2]) + q[:, :, 3]
    o = POOL_TREE // 2
    while o:
        p = p[:, :o] + p[:, o:2 * o]
        o //= 2
    ss = p[:, 0]
    ok = (ss > 0) & torch.isfinite(ss)
    r = torch.sqrt(torch.where(ok, ss, torch.ones_like(ss)))
    d = (md / r[:, None]).to(torch.float32).to(torch.bfloat16)
    return torch.where(ok[:, None], d, torch.zeros_like(d))


def rows_pool(y, row_off, lo=0, hi=None, out=None, row_off_host=None):
    """The prescreen descriptors of the entries [lo, hi) of a ragged row store (fpm_rows_pool) -> (hi - lo, 768)
    bf16: y (R, 768) fp32 and row_off (G + 1,) int64 on one device (entry g = rows row_off[g] .. row_off[g + 1]);
    ``hi`` None: G.  Per entry of n rows:

        m[c] = the fp32 sum of y[i, c] over i ascending, one running sum per channel from +0.0;
        ss   = the fp64 sum of double(m[c])^2 in a fixed order: p[t] = ((m[4t]^2 + m[4t+1]^2) + m[4t+2]^2) +
               m[4t+3]^2 for t < POOL_THREADS = 192, p[192 .. 256) = 0, then for o = 128, 64, .. 1:
               p[t] += p[t + o] for t < o; ss = p[0];
        r    = sqrt(ss) in fp64;  d[c] = bf16_rne(float(double(m[c]) / r)).

    ss == 0 or not finite gives an all-zero descriptor.  Every step is one correctly rounded IEEE operation, so
    the kernel (device tensors) and the statement above in torch (CPU tensors) give the same bits.  Checked on
    the host before anything is launched: dtypes, contiguity, devices, 0 <= lo <= hi <= G and offsets that rise
    from 0 to R (``row_off_host``: a host copy, so the check needs no device synchronisation)."""
    op = "rows_pool"
    _check_row_store(op, "y", y)
    _check_index_tensors(op, (("row_off", row_off, torch.int64),))
    _check_on_device_of(op, y, (("row_off", row_off), ("out", out)))
    G = int(row_off.numel()) - 1
    if G < 0:
        raise _lib.FpmError("%s: row_off must hold G + 1 >= 1 offsets" % op)
    hi = G if hi is None else int(hi)
    lo = int(lo)
    if not 0 <= lo <= hi <= G:
        raise _lib.FpmError("%s: entries [%d, %d) outside the index's [0, %d]" % (op, lo, hi, G))
    oh = _host_copy(row_off_host, row_off)
    if oh.numel() != G + 1 or not _offsets_rise(oh, y):
        raise _lib.FpmError("%s: row_off must rise from 0 to the %d rows of y" % (op, y.shape[0]))
    out = _out_tensor(op, "out", out, (hi - lo, DESC_DIM), torch.bfloat16, y.device,
                      "out must be a contiguous bfloat16 tensor")
    if hi == lo:
        return out
    if y.data_ptr() & 15 or out.data_ptr() & 7:
        raise _lib.FpmError("%s: y must be 16-byte aligned, out 8-byte aligned" % op)
    if not y.is_cuda:
        return out.copy_(_rows_pool_host(y, oh[lo:hi + 1]))
    _lib.call("fpm_rows_pool", _p(y), int(y.shape[0]), _p(row_off), lo, hi, _p(out), _stream(y))
    return out


def _desc_score_host(dq, dg, dtype):
    """score[q, b] = sum_c dq[q, c] dg[b, c] in ``dtype`` arithmetic, c ascending, one product and one add per
    channel (a product of two bf16 values is exact in fp32)."""
    a, b = dq.to(dtype), dg.to(dtype)
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=dtype)
    for c in range(DESC_DIM):
        acc = acc + a[:, c, None] * b[None, :, c]
    return acc


def desc_score(dq, dg, idx=None, out=None, idx_host=None, dtype=None):
    """Descriptor scores, probes x entries (fpm_desc_score) -> (Q, B) fp32: score[q, b] = sum_c dq[q, c] *
    dg[idx[b], c] for descriptors dq (Q, 768) and dg (G, 768) bf16 (``rows_pool``); ``idx`` (B,) int32 selects
    entries, None means all G in order.  The kernel accumulates in fp32 on v_mfma_f32_16x16x32_bf16, the 24 K steps
    ascending, probes in tiles of 16: a score's bits depend on its (probe, entry) pair alone, not on the other
    probes, the other entries or the pair's place in ``idx``.  Checked on the host before anything is launched:
    dtypes, contiguity, devices, 16-byte alignment, and every idx in [0, G) when ``idx_host`` (a host copy) is given
    or the tensors are on the host; the kernel itself reads nothing for an idx outside [0, G) and writes NaN.

    CPU tensors take the statement: the sum over ascending c in ``dtype`` arithmetic (torch.float32, the default,
    or torch.float64), to which the kernel agrees within rounding (the MFMA's order inside a K step is its own)."""
    op = "desc_score"
    for name, t in (("dq", dq), ("dg", dg)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.bfloat16 or t.dim() != 2 or t.shape[1] != DESC_DIM \
                or not t.is_contiguous():
            raise _lib.FpmError("%s: %s must be contiguous bfloat16 descriptors of 768 channels" % (op, name))
    if idx is not None:
        _check_index_tensors(op, (("idx", idx, torch.int32),))
    _check_on_device_of(op, dq, (("dg", dg), ("idx", idx), ("out", out)))
    Q, G = int(dq.shape[0]), int(dg.shape[0])
    B = G if idx is None else int(idx.numel())
    if Q > 16 * 65535:
        raise _lib.FpmError("%s: at most %d probes per call" % (op, 16 * 65535))
    if idx is not None and (idx_host is not None or not dq.is_cuda):
        ih = _host_copy(idx_host, idx)
        if ih.numel() != B:
            raise _lib.FpmError("%s: the host copy of idx does not match the device tensor" % op)
        if B and (int(ih.min()) < 0 or int(ih.max()) >= G):
            raise _lib.FpmError("%s: idx value outside [0, %d)" % (op, G))
    if not dq.is_cuda:
        dtype = _host_dtype(op, dtype)
        res = _desc_score_host(dq, dg if idx is None else dg[idx.long()], dtype)
        if out is None:
            return res
        _shape(out, (Q, B), "%s out" % op)
        return out.copy_(res)
    if dtype is not None:
        raise _lib.FpmError("%s: dtype selects the host statement's arithmetic; the kernel is fp32" % op)
    out = _out_tensor(op, "out", out, (Q, B), torch.float32, dq.device, "out must be contiguous fp32")
    if Q == 0 or B == 0:
        return out
    if (dq.data_ptr() | dg.data_ptr()) & 15:
        raise _lib.FpmError("%s: dq and dg must be 16-byte aligned" % op)
    _lib.call("fpm_desc_score", _p(dq), Q, _p(dg), G, _p(idx), B, _p(out), _stream(dq))
    return out


TOPK_MERGE_SMAX = 16


def topk_merge(score, ids, list_off, k, top_id=None, top_score=None, top_col=None):
    """Per row, the k best of S sorted candidate lists (fpm_topk_merge; a gallery spread over several
    devices merges its shards' shortlists with it).  score (P, L) fp32 and ids (P, L) int32 >= 0 (any row
    stride, the columns dense); ``list_off``: S + 1 host integers rising from 0 to L, list t the columns
    [list_off[t], list_off[t + 1]), possibly empty; S <= 16, a list at most 1024 long, P <= 65535,
    1 <= k <= min(L, 1024).  The key of a candidate is ``rank_key(score, ids)``: ``rank_select``'s key with the
    id in place of the column, so ties go to the lower id.  Precondition: every list strictly descending by
    key, the ids of a row distinct.
    -> (top_id (P, k) int32, top_score (P, k) fp32, top_col (P, k) int32): the k largest keys, descending:
    their ids, scores (the same bits) and columns (caller-allocated on the device path when given).

    CPU tensors take the statement: a stable descending sort of the key; the precondition is checked there
    and a violation raises.  Device tensors run the kernel, which equals the statement bit for bit and does
    not check the precondition (it stays inside its buffers whatever the data)."""
    op = "topk_merge"
    P, L = _check_scores(op, score, "score", "(P, L)")
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or tuple(ids.shape) != tuple(score.shape):
        raise _lib.FpmError("%s: ids must be an int32 tensor of score's shape %s" % (op, tuple(score.shape)))
    if ids.device != score.device:
        raise _lib.FpmError("%s: ids is on %s, score on %s" % (op, ids.device, score.device))
    off = torch.as_tensor(list_off).detach().cpu().view(-1)
    if off.dtype not in (torch.int64, torch.int32) or off.numel() < 2:
        raise _lib.FpmError("%s: list_off must be S + 1 >= 2 host integers" % op)
    off = off.to(torch.int64)
    S = int(off.numel()) - 1
    if S > TOPK_MERGE_SMAX:
        raise _lib.FpmError("%s: S = %d lists, at most %d" % (op, S, TOPK_MERGE_SMAX))
    length = off[1:] - off[:-1]
    if int(off[0]) != 0 or bool((length < 0).any()):
        raise _lib.FpmError("%s: list_off must start at 0 and must not fall" % op)
    if int(length.max()) > RANK_SELECT_KMAX:
        raise _lib.FpmError("%s: a list of %d candidates, at most %d" % (op, int(length.max()), RANK_SELECT_KMAX))
    if int(off[-1]) != L:
        raise _lib.FpmError("%s: list_off ends at %d, a row holds %d candidates" % (op, int(off[-1]), L))
    k = int(k)
    if not 1 <= k <= min(L, RANK_SELECT_KMAX):
        raise _lib.FpmError("%s: k = %d outside [1, min(L, %d) = %d]" % (op, k, RANK_SELECT_KMAX, min(L, RANK_SELECT_KMAX)))
    if P > 65535:
        raise _lib.FpmError("%s: at most 65535 rows per call" % op)
    if not score.is_cuda:
        if P and int(ids.min()) < 0:
            raise _lib.FpmError("%s: a negative id" % op)
        keys = rank_key(score, ids)
        inner = torch.ones(L, dtype=torch.bool)
        inner[off[:-1][length > 0]] = False                      # a list's first column has no left neighbour
        if P and L > 1 and bool(((keys[:, 1:] >= keys[:, :-1]) & inner[1:]).any()):
            raise _lib.FpmError("%s: a list is not strictly descending by key" % op)
        srt = torch.sort(ids, dim=1).values
        if P and L > 1 and bool((srt[:, 1:] == srt[:, :-1]).any()):
            raise _lib.FpmError("%s: an id twice in one row" % op)
        col = torch.argsort(keys, dim=1, descending=True, stable=True)[:, :k]
        return torch.gather(ids, 1, col), torch.gather(score, 1, col), col.to(torch.int32)
    if L > 1 and (score.stride(1) != 1 or ids.stride(1) != 1):
        score, ids = score.contiguous(), ids.contiguous()
    ld = int(score.stride(0)) if P > 1 else L
    if ld < L or (P > 1 and int(ids.stride(0)) != ld):
        score, ids, ld = score.contiguous(), ids.contiguous(), L
    top_id, top_score, top_col = (
        _out_tensor(op, name, t, (P, k), dt, score.device, "%s must be contiguous %s on score's device" % (name, dt))
        for name, t, dt in (("top_id", top_id, torch.int32), ("top_score", top_score, torch.float32),
                            ("top_col", top_col, torch.int32)))
    if P == 0:
        return top_id, top_score, top_col
    offs = (ctypes.c_int * (S + 1))(*off.tolist())
    _lib.call("fpm_topk_merge", _p(score), _p(ids), ld, P, offs, S, k, _p(top_id), _p(top_score), _p(top_col),
              _stream(score))
    return top_id, top_score, top_col


GROUP_FUSE = ("max", "mean")
# GRP_TEAM and GRP_WIDE of csrc/rank_groups.h: the host statements sum in the order these fix
GROUP_TEAM = 16                 # lanes that sum a group of at most GROUP_WIDE entries
GROUP_WIDE = 1024               # larger groups are summed by 64 lanes


def _group_rows_host(scores, off, pos, mean, gscore, gbest):
    """The statement of fpm_group_scores for rows that share one structure: scores (R, G) fp32, off
    (S + 1,) and pos int64 host tensors (checked by the caller), into gscore / gbest (R, S).

    gbest: the group's position with the largest ``rank_key``.  Max: the score there.  Mean, for a
    group of c entries x[0..c) (x[j] = scores[r, pos[off[s] + j]]): W = GROUP_TEAM lanes for
    c <= GROUP_WIDE, else 64; lane t starts from +0.0 and adds x[t], x[t + W], ... in order (a lane past
    the group's end adds +0.0, which changes no bit: a lane's value is never -0.0); then for
    m = W/2 .. 1 every lane takes v + v[lane ^ m]; lane 0's value over fp32(c), NaN as 0x7FC00000."""
    R = int(scores.shape[0])
    keys = rank_key(scores) if R else scores.new_zeros(scores.shape, dtype=torch.int64)
    cnt = off[1:] - off[:-1]
    width = torch.where(cnt > GROUP_WIDE, 64, GROUP_TEAM)
    rounds = (cnt + width - 1) // width
    qnan = torch.full((), float("nan"), dtype=torch.float32)
    gscore.copy_(qnan.expand_as(gscore))
    gbest.fill_(-1)
    for w, r in sorted(set(zip(width[cnt > 0].tolist(), rounds[cnt > 0].tolist()))):
        gs = torch.nonzero((width == w) & (rounds == r) & (cnt > 0)).view(-1)
        j = torch.arange(r * w, dtype=torch.int64).view(1, -1)
        valid = j < cnt[gs].view(-1, 1)
        at = pos[torch.where(valid, off[gs].view(-1, 1) + j, torch.zeros((), dtype=torch.int64))]       # (ng, r * w)
        k = torch.where(valid.unsqueeze(0), keys[:, at], torch.full((), -2 ** 63, dtype=torch.int64))
        best = 0xFFFFFFFF - (k.max(dim=2).values & 0xFFFFFFFF)                                       # (R, ng)
        gbest[:, gs] = best.to(torch.int32)
        if not mean:
            gscore[:, gs] = torch.gather(scores, 1, best)
            continue
        x = torch.where(valid.unsqueeze(0), scores[:, at], torch.zeros((), dtype=torch.float32)).view(R, -1, r, w)
        acc = torch.zeros(R, int(gs.numel()), w, dtype=torch.float32)
        for i in range(r):
            acc = acc + x[:, :, i, :]
        lanes = torch.arange(w)
        m = w // 2
        while m:
            acc = acc + acc[..., lanes ^ m]
            m //= 2
        val = acc[..., 0] / cnt[gs].to(torch.float32).view(1, -1)
        gscore[:, gs] = torch.where(torch.isnan(val), qnan, val)


def group_scores(scores, off, pos, fuse="max", gscore=None, gbest=None, off_host=None, pos_host=None):
    """Per-group fusion of a score matrix (fpm_group_scores; a group is the impressions of one subject):
    scores (P, G) fp32 (any row stride); CSR tables ``off`` (S + 1,) int32 rising from 0 and ``pos`` int32
    positions into a row of scores, group s = pos[off[s]:off[s + 1]] -- one structure shared by all
    rows, or one per row: off (P, S + 1), pos (P, L), row p's positions at pos[p, :off[p, S]] (the rest
    of the row is padding).  Positions need not cover the row; a group may be empty.
    -> (gscore (P, S) fp32, gbest (P, S) int32).

    gbest: the group's position with the largest ``rank_key`` (the key built from the position): the best
    score, ties to the lower position, NaN below every number (an all-NaN group: its lowest position).
    fuse="max": gscore = scores[p, gbest], the same bits.  fuse="mean": the fp32 sum of the group's
    entries in the fixed order ``_group_rows_host`` states, over fp32(count), correctly rounded; NaN and
    infinities propagate, a NaN mean is the canonical 0x7FC00000.  An empty group: NaN, -1.  A group's
    result depends on its own entries and their order alone: not on P, S or the other groups.

    Device tensors run the kernel; CPU tensors take the statement, which the kernel equals bit for bit.
    Refused before any launch: dtypes, shapes, devices, offsets that do not start at 0, fall or pass
    the end of pos, a used position outside [0, G), P > 65535 (``off_host`` / ``pos_host``: host copies,
    so the check needs no device synchronisation; without them the device tensors are copied back)."""
    if fuse not in GROUP_FUSE:
        raise _lib.FpmError("group_scores: fuse must be one of %s" % (GROUP_FUSE,))
    mean = fuse == "mean"
    return _group_op("group_scores", "fpm_group_scores", int(mean), scores, off, pos, gscore, gbest, off_host, pos_host,
                     lambda s, o, p, gs, gb: _group_rows_host(s, o, p, mean, gs, gb))


def _group_op(op, entry, arg, scores, off, pos, gscore, gbest, off_host, pos_host, rows_host):
    """The checks and the CPU / GPU dispatch shared by ``group_scores`` and ``group_topr``: ``entry`` is the
    C-ABI function, ``arg`` its one integer besides the structures (the fuse, or r), ``rows_host(scores (R, G),
    off, pos, gscore, gbest)`` the statement for rows that share one structure."""
    P, G = _check_scores(op, scores)
    if G < 1:
        raise _lib.FpmError("%s: scores has no columns" % op)
    for name, t in (("off", off), ("pos", pos)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
            raise _lib.FpmError("%s: %s must be a int32 tensor (got %s)" % (op, name, getattr(t, "dtype", type(t).__name__)))
        if not t.is_contiguous():
            raise _lib.FpmError("%s: %s must be contiguous" % (op, name))
        if t.device != scores.device:
            raise _lib.FpmError("%s: %s is on %s, scores on %s" % (op, name, t.device, scores.device))
    per_row = off.dim() == 2
    if off.dim() not in (1, 2) or pos.dim() != off.dim() or off.shape[-1] < 1:
        raise _lib.FpmError("%s: off (S + 1,) with pos (L,) for a shared structure, or off (P, S + 1) with pos (P, L)" % op)
    S = int(off.shape[-1]) - 1
    if per_row and (int(off.shape[0]) != P or int(pos.shape[0]) != P or int(pos.shape[1]) < 1):
        raise _lib.FpmError("%s: per-row structures need off (%d, S + 1) and pos (%d, L >= 1)" % (op, P, P))
    if P > 65535:
        raise _lib.FpmError("%s: at most 65535 rows per call" % op)
    oh = torch.as_tensor(off_host if off_host is not None else off.cpu()).long()
    ph = torch.as_tensor(pos_host if pos_host is not None else pos.cpu()).long()
    if tuple(oh.shape) != tuple(off.shape) or tuple(ph.shape) != tuple(pos.shape):
        raise _lib.FpmError("%s: host copies of off / pos do not match the device tensors" % op)
    oh2, ph2 = oh.view(-1, S + 1), ph.view(oh.numel() // (S + 1), -1)
    L = int(ph2.shape[1])
    if oh2.numel() and (bool((oh2[:, 0] != 0).any()) or bool((oh2[:, 1:] < oh2[:, :-1]).any())):
        raise _lib.FpmError("%s: offsets must start at 0 and must not fall" % op)
    if oh2.numel() and int(oh2[:, -1].max()) > L:
        raise _lib.FpmError("%s: offsets end at %d, pos holds %d positions" % (op, int(oh2[:, -1].max()), L))
    used = torch.arange(L).view(1, -1) < oh2[:, -1:]
    if bool((used & ((ph2 < 0) | (ph2 >= G))).any()):
        raise _lib.FpmError("%s: a position outside [0, %d)" % (op, G))
    msg = "gscore must be contiguous fp32, gbest contiguous int32, on the scores' device"
    gscore = _out_tensor(op, "gscore", gscore, (P, S), torch.float32, scores.device, msg)
    gbest = _out_tensor(op, "gbest", gbest, (P, S), torch.int32, scores.device, msg)
    if P == 0 or S == 0:
        return gscore, gbest
    if L == 0:                                   # no positions at all: every group is empty
        gscore.fill_(float("nan"))
        gbest.fill_(-1)
        return gscore, gbest
    if not scores.is_cuda:
        if per_row:
            for p in range(P):
                rows_host(scores[p:p + 1], oh2[p], ph2[p], gscore[p:p + 1], gbest[p:p + 1])
        else:
            rows_host(scores, oh2[0], ph2[0], gscore, gbest)
        return gscore, gbest
    scores, ld = _dense_rows(scores)
    _lib.call(entry, _p(scores), ld, P, G, _p(off), S + 1 if per_row else 0, _p(pos), L if per_row else 0, S,
              int(arg), _p(gscore), _p(gbest), _stream(scores))
    return gscore, gbest


TOPR_MAX = 16


def _topr_rows_host(scores, off, pos, r, gscore, gbest):
    """The statement of fpm_group_topr for rows that share one structure (arguments as ``_group_rows_host``).

    gbest: ``_group_rows_host``'s.  gscore, for a group of c >= 1 entries x[0..c): r' = min(r, c); the entries
    in descending order of their score's ``rank_key`` bits (NaN last; a stable sort, though entries that tie
    have one value, so their order changes no bit); s = +0.0, then s = s + x1, ..., s = s + x_r', each one
    fp32 addition; s / fp32(r'), NaN as 0x7FC00000."""
    R = int(scores.shape[0])
    _group_rows_host(scores, off, pos, False, gscore, gbest)            # gbest; gscore is overwritten below
    bits = (rank_key(scores) >> 32) if R else scores.new_zeros(scores.shape, dtype=torch.int64)
    cnt = off[1:] - off[:-1]
    qnan = torch.full((), float("nan"), dtype=torch.float32)
    for c in sorted(set(cnt[cnt > 0].tolist())):
        gs = torch.nonzero(cnt == c).view(-1)
        at = pos[off[gs].view(-1, 1) + torch.arange(c, dtype=torch.int64).view(1, -1)]          # (ng, c)
        order = torch.sort(bits[:, at], dim=2, descending=True, stable=True).indices[..., :min(r, c)]
        x = torch.gather(scores[:, at], 2, order)                                               # (R, ng, r')
        acc = torch.zeros(R, int(gs.numel()), dtype=torch.float32)
        for i in range(min(r, c)):
            acc = acc + x[..., i]
        val = acc / torch.full((), float(min(r, c)), dtype=torch.float32)
        gscore[:, gs] = torch.where(torch.isnan(val), qnan, val)


def group_topr(scores, off, pos, r, gscore=None, gbest=None, off_host=None, pos_host=None):
    """The mean of each group's r best entries (fpm_group_topr; open-set search: a genuine subject's score
    rests on its r best impressions, a bad one does not sink it).  Arguments, structures, refusals and
    dispatch as ``group_scores``; 1 <= r <= TOPR_MAX -> (gscore (P, S) fp32, gbest (P, S) int32).

    gbest: ``group_scores``'s.  gscore of a group of c >= 1 entries: r' = min(r, c), the r' entries with the
    largest ``rank_key`` in descending order x1 .. x_r', s = +0.0, s = s + x1, ..., s = s + x_r' (fp32
    additions in that order), s / fp32(r') correctly rounded; NaN ranks last, so it enters (and propagates)
    only when the group holds fewer than r' numbers; infinities propagate; a NaN result is 0x7FC00000.  r = 1
    is the max as a number (the bits differ where the best is -0.0, which 0.0 + -0.0 turns into +0.0, or a
    NaN with other bits).  An empty group: NaN, -1.  A group's result depends on its own entries and their order
    alone.  Device tensors run the kernel; CPU tensors take the statement (``_topr_rows_host``), which the
    kernel equals bit for bit."""
    if isinstance(r, bool) or not isinstance(r, int) or not 1 <= r <= TOPR_MAX:
        raise _lib.FpmError("group_topr: r = %r outside [1, %d] (an integer)" % (r, TOPR_MAX))
    return _group_op("group_topr", "fpm_group_topr", r, scores, off, pos, gscore, gbest, off_host, pos_host,
                     lambda s, o, p, gs, gb: _topr_rows_host(s, o, p, r, gs, gb))


COHORT_WINDOW = 1024            # skip + cohort at most: 16 strided rounds of 64 lanes


def _lane_sum64(v):
    """L(v) of ``cohort_decide`` over the last dimension (a multiple of 64, padded with +0.0): 64 lanes, lane t
    starts from +0.0 and adds v[t], v[t + 64], ... in order; then for m = 32 .. 1 every lane takes
    v + v[lane ^ m]; lane 0's value.  (``_group_rows_host``'s order with W = 64 always; a padding +0.0 changes
    no bit: a lane's value is never -0.0.)"""
    v = v.view(v.shape[0], -1, 64)
    acc = torch.zeros(v.shape[0], 64, dtype=torch.float32)
    for i in range(v.shape[1]):
        acc = acc + v[:, i, :]
    lanes = torch.arange(64)
    m = 32
    while m:
        acc = acc + acc[:, lanes ^ m]
        m //= 2
    return acc[:, 0]


def _cohort_host(top, k, skip, cohort, sigma_floor):
    """The statement of fpm_cohort_decide's statistics and z-scores on a CPU tensor -> (z (P, k), mu, sigma (P,),
    n (P,) int32).  Every line is one rounded fp32 operation per element; the square is a product of its own,
    not fused into the sum."""
    P, K = int(top.shape[0]), int(top.shape[1])
    qnan = torch.full((), float("nan"), dtype=torch.float32)
    win = top[:, skip:min(K, skip + cohort)]
    W = int(win.shape[1])
    pad = max(1, (W + 63) // 64) * 64
    ok = ~torch.isnan(win)
    n = ok.sum(1)
    # the non-NaN values in column order, then +0.0 up to a multiple of 64
    front = torch.argsort((~ok).to(torch.int8), dim=1, stable=True)
    x = torch.zeros(P, pad, dtype=torch.float32)
    live = torch.zeros(P, pad, dtype=torch.bool)
    x[:, :W] = torch.where(torch.arange(W).view(1, -1) < n.view(-1, 1), torch.gather(win, 1, front),
                           torch.zeros((), dtype=torch.float32))
    live[:, :W] = torch.arange(W).view(1, -1) < n.view(-1, 1)
    fn = n.clamp(min=1).to(torch.float32)
    mu = _lane_sum64(x) / fn
    d = x - mu.view(-1, 1)
    q = torch.where(live, d * d, torch.zeros((), dtype=torch.float32))
    var = _lane_sum64(q) / fn
    # the correctly rounded fp32 root by way of float64 (53 >= 2 * 24 + 2 bits: rounding twice is exact for a square
    # root); torch's own fp32 sqrt is a vector-library call on some hosts, within an ulp but not correctly rounded
    sigma = torch.sqrt(var.to(torch.float64)).to(torch.float32)
    mu = torch.where((n < 2) | torch.isnan(mu), qnan, mu)
    sigma = torch.where((n < 2) | torch.isnan(sigma), qnan, sigma)
    s = torch.where(torch.isnan(sigma), qnan, torch.maximum(sigma, torch.full((), sigma_floor, dtype=torch.float32)))
    z = (top[:, :k] - mu.view(-1, 1)) / s.view(-1, 1)
    return torch.where(torch.isnan(z), qnan, z), mu, sigma, n.to(torch.int32)


def cohort_decide(top, k, skip=1, cohort=32, sigma_floor=1e-6, threshold=None, normalize=True):
    """z-scores of ranked rows against their own impostor cohorts, and an accept decision (fpm_cohort_decide;
    open-set search: scores are not comparable from probe to probe, a probe's candidates are judged against that
    probe's next-best candidates).  top (P, K) fp32 contiguous, each row as ``rank_select`` returns it (descending,
    NaN last); 1 <= k <= K, skip >= 0, cohort >= 2, skip + cohort <= COHORT_WINDOW
    -> (z (P, k) fp32, mu (P,), sigma (P,), n (P,) int32, accept (P, k) int32), None for the parts not asked for:
    ``normalize=False`` computes no statistics (z, mu, sigma, n are None), ``threshold=None`` no accept.

    Row p's cohort: the non-NaN values among columns skip <= j < min(K, skip + cohort), in column order,
    x[0..n).  mu = L(x) / fp32(n) (L: ``_lane_sum64``), d_j = x_j - mu, q_j = d_j * d_j, var = L(q) / fp32(n),
    sigma = sqrt(var), each a single rounded fp32 operation; n < 2: mu = sigma = NaN and every z is NaN.
    s = max(sigma, sigma_floor) (NaN if sigma is), z_j = (top[p, j] - mu) / s.  accept_j = (v_j >= threshold),
    v = z, or top with ``normalize=False``; a NaN never accepts; 0 / 1.  ``sigma_floor`` and ``threshold`` are
    taken as fp32.  Every NaN returned is 0x7FC00000.

    CPU tensors take the statement (``_cohort_host``), device tensors the kernel, which equals it bit for bit.
    Refused before any launch: dtype, shape, contiguity, the ranges above, a NaN threshold, a sigma_floor that is not a positive finite fp32 number, nothing asked for, P > 65535."""
    op = "cohort_decide"
    if not isinstance(top, torch.Tensor) or top.dim() != 2 or top.dtype != torch.float32:
        raise _lib.FpmError("%s: top must be a (P, K) fp32 tensor" % op)
    if not top.is_contiguous():
        raise _lib.FpmError("%s: top must be contiguous" % op)
    P, K = int(top.shape[0]), int(top.shape[1])
    for name, v in (("k", k), ("skip", skip), ("cohort", cohort)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise _lib.FpmError("%s: %s must be an integer (got %r)" % (op, name, v))
    if not 1 <= k <= K:
        raise _lib.FpmError("%s: k = %d outside [1, K = %d]" % (op, k, K))
    if skip < 0 or cohort < 2 or skip + cohort > COHORT_WINDOW:
        raise _lib.FpmError("%s: skip = %d, cohort = %d (skip >= 0, cohort >= 2, skip + cohort <= %d)"
                            % (op, skip, cohort, COHORT_WINDOW))
    if not normalize and threshold is None:
        raise _lib.FpmError("%s: nothing to compute (normalize=False and threshold=None)" % op)
    floor32 = float(torch.tensor(float(sigma_floor), dtype=torch.float32))
    if normalize and not 0.0 < floor32 < float("inf"):
        raise _lib.FpmError("%s: sigma_floor must be a positive finite fp32 number (got %r)" % (op, sigma_floor))
    thr32 = None
    if threshold is not None:
        thr32 = float(torch.tensor(float(threshold), dtype=torch.float32))
        if thr32 != thr32:
            raise _lib.FpmError("%s: threshold is NaN" % op)
    if P > 65535:
        raise _lib.FpmError("%s: at most 65535 rows per call" % op)
    if not top.is_cuda:
        z = mu = sigma = n = accept = None
        if normalize:
            z, mu, sigma, n = _cohort_host(top, k, skip, cohort, floor32)
        if thr32 is not None:
            accept = ((z if normalize else top[:, :k]) >= thr32).to(torch.int32)
        return z, mu, sigma, n, accept
    new = lambda shape, dt: torch.empty(shape, device=top.device, dtype=dt)
    z = mu = sigma = n = accept = None
    if normalize:
        z, mu, sigma, n = new((P, k), torch.float32), new((P,), torch.float32), new((P,), torch.float32), new((P,), torch.int32)
    if thr32 is not None:
        accept = new((P, k), torch.int32)
    if P:
        _lib.call("fpm_cohort_decide", _p(top), P, K, k, skip, cohort, floor32 if normalize else 1.0, int(bool(normalize)),
                  int(thr32 is not None), 0.0 if thr32 is None else thr32, _p(z), _p(mu), _p(sigma), _p(n), _p(accept),
                  _stream(top))
    return z, mu, sigma, n, accept


COARSE_NMAX = 128
COARSE_WIDE_NMAX = 256         # ``coarse_score_wide``: the block in registers
COARSE_STREAM_NMAX = 600        # ``coarse_score_stream``: the block streamed from a workspace (the matcher's cap)


def _bf16_rne(t):
    """fp32 -> the nearest bf16 value (ties to even), as fp32."""
    return t.to(torch.bfloat16).to(torch.float32)


def _coarse_score_host(y, row_off, idx, yp, coef, iters, tau, dtype):
    """The definition of the coarse score in plain torch (``dtype`` fp32 or fp64 arithmetic on the
    bf16-rounded operands): Kp = softplus(a b^T) - 0.5, pygmtools' log Sinkhorn with dummy rows,
    sum P o Kp / min(n0, n_g)."""
    n0 = int(yp.shape[0])
    out = torch.empty(int(idx.numel()), dtype=dtype)
    for b, g in enumerate(idx.tolist()):
        r0, r1 = int(row_off[g]), int(row_off[g + 1])
        a = _bf16_rne(yp * coef[b]).to(dtype)                 # one fp32 multiply, rounded once
        bm = _bf16_rne(y[r0:r1]).to(dtype)
        Kp = torch.nn.functional.softplus(a @ bm.t()) - 0.5
        L = Kp / tau
        r, c = n0, r1 - r0
        if r > c:
            L, r, c = L.t(), c, r
        if c > r:
            L = torch.cat([L, torch.full((c - r, c), -100.0, dtype=dtype)], 0)
        for i in range(iters):
            L = L - torch.logsumexp(L, 1 if i % 2 == 0 else 0, keepdim=True)
            L = torch.where(torch.isnan(L), torch.full_like(L, -float("inf")), L)
        Pm = torch.exp(L[:r])
        if n0 > r1 - r0:
            Pm = Pm.t()
        out[b] = (Pm * Kp).sum() / min(n0, r1 - r0)
    return out


# The coarse kernels by route name (``gallery.coarse_routes`` numbers them in this order): the C symbol of the
# one-probe and of the pair-list entry point, the size bound's name and value, and how many of
# (B, n0max, ngmax) the kernel's ``<one-probe symbol>_ws_bytes`` takes (0: no workspace).
_COARSE_KERNELS = {"fused": ("fpm_coarse_score", "fpm_coarse_pairs", "COARSE_NMAX", COARSE_NMAX, 0),
                   "wide": ("fpm_coarse_score_wide", "fpm_coarse_pairs_wide", "COARSE_WIDE_NMAX", COARSE_WIDE_NMAX, 1),
                   "stream": ("fpm_coarse_score_stream", "fpm_coarse_pairs_stream", "COARSE_STREAM_NMAX",
                              COARSE_STREAM_NMAX, 3)}
COARSE_KERNELS = tuple(_COARSE_KERNELS)


def _coarse_call(kernel, pairs, y, args, B, n0max, ngmax):
    """Launch ``kernel``'s one-probe or pair-list (``pairs``) entry point for the index rows ``y`` (fp32, or
    their bf16 copy: the _rows16 symbols, or their fp8 form: the _rows8 symbols, whose ``args`` begin with
    the rows and their scales) with ``args``, its workspace (sized from the launch's largest probe
    and largest entry, allocated here on the caller's stream) and the stream."""
    one, many, _, _, nws = _COARSE_KERNELS[kernel]
    rows = {torch.float32: "", torch.bfloat16: "_rows16", torch.float8_e4m3fn: "_rows8"}[y.dtype]
    ws = ()
    if nws:
        buf, wsb = _scratch(one + "_ws_bytes", y.device, *(B, n0max, ngmax)[:nws])
        ws = (_p(buf), wsb)
    _lib.call((many if pairs else one) + rows, *args, *ws, _stream(y))


# The checks and prologues that the ranking, ``coarse_score*``, ``coarse_pairs`` and ``rows_*`` wrappers make
# alike; ``op`` names the caller in the message.  (The device checks of ``rows_fetch`` / ``rows_pack`` word theirs
# after other tensors -- "out on", "src on" -- and stay with them.)
def _check_index_tensors(op, named):
    for name, t, dt in named:
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise _lib.FpmError("%s: %s must be a %s tensor (got %s)"
                                % (op, name, str(dt).replace("torch.", ""), getattr(t, "dtype", type(t).__name__)))
        if t.dim() != 1 or not t.is_contiguous():
            raise _lib.FpmError("%s: %s must be a contiguous 1-d tensor" % (op, name))


def _check_coarse_rows(op, y, named, row_scale=None):
    # y: the index's fp32 rows, their bf16 copy (an index's y16: the rounding already done) or their fp8 form
    # with ``row_scale`` (an index's y8 and s8: ``rows_quant8``)
    if not isinstance(y, torch.Tensor) or y.dtype not in (torch.float32, torch.bfloat16, torch.float8_e4m3fn) \
            or y.dim() != 2 or y.shape[1] != DESC_DIM or not y.is_contiguous():
        raise _lib.FpmError("%s: y must be contiguous fp32 or bf16 rows of 768 channels (or float8_e4m3fn rows with "
                            "row_scale=)" % op)
    if (y.dtype == torch.float8_e4m3fn) != (row_scale is not None):
        raise _lib.FpmError("%s: float8_e4m3fn rows y go with their scales row_scale=, other rows without" % op)
    if row_scale is not None:
        if not isinstance(row_scale, torch.Tensor) or row_scale.dtype != torch.float32:
            raise _lib.FpmError("%s: row_scale must be a float32 tensor (got %s)"
                                % (op, getattr(row_scale, "dtype", type(row_scale).__name__)))
        if row_scale.dim() != 1 or not row_scale.is_contiguous() or row_scale.numel() != y.shape[0]:
            raise _lib.FpmError("%s: row_scale must be a contiguous 1-d tensor of one scale per row of y (%d)"
                                % (op, y.shape[0]))
        if row_scale.device != y.device:
            raise _lib.FpmError("%s: row_scale is on %s, y on %s" % (op, row_scale.device, y.device))
    for name, t in named:
        _check_row_store(op, name, t)


def _check_on_device_of(op, y, named):
    for name, t in named:
        if t is not None and t.device != y.device:
            raise _lib.FpmError("%s: %s is on %s, y on %s" % (op, name, t.device, y.device))


def _host_copy(host, t):
    return torch.as_tensor(host if host is not None else t.cpu()).view(-1).long()


def _offsets_rise(off, rows):
    """Host offsets ``off`` rise from 0 to the row count of ``rows``."""
    return int(off[0]) == 0 and int(off[-1]) == rows.shape[0] and not bool((off[1:] < off[:-1]).any())


def _check_selection(op, idx, row_off, rows, rows_name, idx_host, row_off_host):
    """A selection ``idx`` of the entries of a ragged row store, on host copies (given, or copied back): the copies
    match the tensors, ``row_off`` rises from 0 to the rows of ``rows``, every idx is in [0, G) -> (idx, row_off)
    as host int64."""
    G, B = int(row_off.numel()) - 1, int(idx.numel())
    ih, oh = _host_copy(idx_host, idx), _host_copy(row_off_host, row_off)
    if ih.numel() != B or oh.numel() != G + 1:
        raise _lib.FpmError("%s: host copies of idx / row_off do not match the device tensors" % op)
    if not _offsets_rise(oh, rows):
        raise _lib.FpmError("%s: row_off must rise from 0 to the %d rows of %s" % (op, rows.shape[0], rows_name))
    if B and (int(ih.min()) < 0 or int(ih.max()) >= G):
        raise _lib.FpmError("%s: idx value outside [0, %d)" % (op, G))
    return ih, oh


_ROW_DTYPES = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float8_e4m3fn: "float8_e4m3fn"}


def _check_row_store(op, name, t, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != 2 or t.shape[1] != DESC_DIM \
            or not t.is_contiguous():
        raise _lib.FpmError("%s: %s must be contiguous %s rows of %d channels" % (op, name, _ROW_DTYPES[dtype], DESC_DIM))


def _check_scores(op, scores, name="scores", shape="(P, G)"):
    """A score matrix -> its (P, G)."""
    if not isinstance(scores, torch.Tensor) or scores.dim() != 2 or scores.dtype != torch.float32:
        raise _lib.FpmError("%s: %s must be a %s fp32 tensor" % (op, name, shape))
    return int(scores.shape[0]), int(scores.shape[1])


def _dense_rows(scores):
    """What a kernel reads a (P, G) matrix of any strides through -> (the matrix with dense columns, its row
    stride ld >= G); copied only where the strides ask for it."""
    P, G = int(scores.shape[0]), int(scores.shape[1])
    if G > 1 and scores.stride(1) != 1:
        scores = scores.contiguous()
    ld = int(scores.stride(0)) if P > 1 else G
    if ld < G:
        scores, ld = scores.contiguous(), G
    return scores, ld


def _rank_order(scores, k):
    """The host ranking: every row's first k columns by ``rank_key``, descending (keys are unique)."""
    return torch.argsort(rank_key(scores), dim=1, descending=True, stable=True)[:, :k]


def _out_tensor(op, name, t, shape, dtype, device, msg):
    """An output: a new tensor, or the caller's ``t`` checked -- its shape, then dtype, contiguity and device,
    which the caller words (``msg``)."""
    if t is None:
        return torch.empty(shape, device=device, dtype=dtype)
    if not isinstance(t, torch.Tensor):
        raise _lib.FpmError("%s: %s" % (op, msg))
    _shape(t, shape, "%s %s" % (op, name))
    if t.dtype != dtype or not t.is_contiguous() or t.device != device:
        raise _lib.FpmError("%s: %s" % (op, msg))
    return t


def _scratch(sym, device, *args):
    """Scratch of one call alone, sized by the library's ``sym(*args)`` and allocated on the caller's stream
    -> (uint8 buffer, its size)."""
    wsb = int(getattr(_lib.load(), sym)(*args))
    return torch.empty(wsb, device=device, dtype=torch.uint8), wsb


def _check_iters_tau(op, iters, tau):
    iters, tau = int(iters), float(tau)
    if iters < 0 or not tau > 0:
        raise _lib.FpmError("%s: iters >= 0 and tau > 0 required" % op)
    return iters, tau


def _host_dtype(op, dtype):
    dtype = dtype or torch.float32
    if dtype not in (torch.float32, torch.float64):
        raise _lib.FpmError("%s: the host statement runs in float32 or float64" % op)
    return dtype


def _scale_arg(row_scale):
    """The _rows8 entry points' second argument, after the rows."""
    return () if row_scale is None else (_p(row_scale),)


def _coarse_out(op, y, B, out, dtype, res=None):
    """The (B,) result: ``res`` (the host statement's, CPU tensors) copied to ``out`` if there is one; else
    ``out``, checked or allocated, for the kernel to fill."""
    if res is not None:
        if out is None:
            return res
        _shape(out, (B,), "%s out" % op)
        return out.copy_(res)
    if dtype is not None:
        raise _lib.FpmError("%s: dtype selects the host statement's arithmetic; the kernel is fp32" % op)
    return _out_tensor(op, "out", out, (B,), torch.float32, y.device, "out must be contiguous fp32")


def _coarse_score_op(kernel, y, row_off, idx, yp, coef, iters, tau, out, idx_host, row_off_host, dtype,
                     row_scale=None):
    """``coarse_score``, ``coarse_score_wide`` and ``coarse_score_stream``: the host-side checks, then
    ``kernel``'s one-probe entry point (``_COARSE_KERNELS``; its symbol without "fpm_" names the operation
    in every message)."""
    sym, _, bound, nmax, _ = _COARSE_KERNELS[kernel]
    op = sym[len("fpm_"):]
    _check_index_tensors(op, (("idx", idx, torch.int32), ("row_off", row_off, torch.int64)))
    _check_coarse_rows(op, y, (("yp", yp), ("coef", coef)), row_scale)
    _check_on_device_of(op, y, (("row_off", row_off), ("idx", idx), ("yp", yp), ("coef", coef), ("out", out)))
    G, B, n0 = int(row_off.numel()) - 1, int(idx.numel()), int(yp.shape[0])
    if G < 1:
        raise _lib.FpmError("%s: empty gallery" % op)
    _shape(coef, (B, 768), "%s coef" % op)
    ih, oh = _check_selection(op, idx, row_off, y, "y", idx_host, row_off_host)
    if not 1 <= n0 <= nmax:
        raise _lib.FpmError("%s: a probe of %d keypoints; the coarse pass takes 1 to %s = %d" % (op, n0, bound, nmax))
    if B:
        ng = oh[ih + 1] - oh[ih]
        if int(ng.max()) > nmax or int(ng.min()) < 1:
            raise _lib.FpmError("%s: a selected entry has n_g = %d; the coarse pass takes 1 to "
                                "%s = %d" % (op, int(ng.max()) if int(ng.max()) > nmax else int(ng.min()), bound, nmax))
    iters, tau = _check_iters_tau(op, iters, tau)
    if not y.is_cuda:
        dtype = _host_dtype(op, dtype)
        yh = y if row_scale is None else rows_dequant8(y, row_scale)
        return _coarse_out(op, y, B, out, dtype, _coarse_score_host(yh, oh, ih, yp, coef, iters, tau, dtype))
    out = _coarse_out(op, y, B, out, dtype)
    if B:
        _coarse_call(kernel, False, y, (_p(y), *_scale_arg(row_scale), _p(row_off), _p(idx), G, B, _p(yp), n0, _p(coef),
                                        iters, tau, _p(out)),
                     B, n0, int(ng.max()))
    return out


def coarse_score(y, row_off, idx, yp, coef, iters=10, tau=0.01, out=None, idx_host=None, row_off_host=None,
                 dtype=None, row_scale=None):
    """Coarse 1:N score of one probe against gallery entries idx[b] of a ragged index
    (fpm_coarse_score) -> (B,) fp32:

        a = bf16(yp o coef[b]), b = bf16(y rows of entry idx[b]), Kp = softplus(a b^T) - 0.5,
        P = Sinkhorn(Kp; dummy rows, iters, tau), score[b] = sum P o Kp / min(n0, n_g).

    y (sum n_g, 768) fp32 with row_off int64 [G + 1] and idx int32 [B] as ``rows_gather_scale`` takes
    them, or the same rows as bf16 (``cast_bf16(y)``, an index's ``y16``: the kernel's bf16
    instantiation, fpm_coarse_score_rows16, copies the entry's tile as it is, the same operands and the
    same bits; so for ``coarse_score_wide`` and ``coarse_score_stream``), or the rows as float8_e4m3fn
    with ``row_scale`` (sum n_g,) fp32 (``rows_quant8``, an index's ``y8`` and ``s8``: the _rows8 entry points
    dequantise the entry's tile on the way in, b = bf16(float(y8) * s8), exactly, so the score is the bits of
    the bf16 call on ``rows_dequant8(y8, s8)``); yp (n0, 768) fp32, the
    probe's SplineConv rows; coef (B, 768) fp32 (``coef_tanh``).  Checked
    on the host before anything is launched: dtypes, contiguity and devices, every idx in [0, G),
    n0 and every selected n_g in [1, COARSE_NMAX = 128] (``idx_host`` / ``row_off_host``: host
    copies, so the check needs no device synchronisation).

    CPU tensors take the plain-torch statement of the definition, in ``dtype`` arithmetic
    (torch.float32, the default, or torch.float64) on the same bf16-rounded operands."""
    return _coarse_score_op("fused", y, row_off, idx, yp, coef, iters, tau, out, idx_host, row_off_host, dtype,
                            row_scale)


def coarse_score_wide(y, row_off, idx, yp, coef, iters=10, tau=0.01, out=None, idx_host=None, row_off_host=None,
                      dtype=None, row_scale=None):
    """``coarse_score`` for boxes of up to COARSE_WIDE_NMAX = 256 keypoints (fpm_coarse_score_wide): the
    same definition, arguments and host-side checks, with n0 and every selected n_g in
    [1, COARSE_WIDE_NMAX].  The kernel keeps the block in registers and parks Kp in a scratch of
    min(B, 256) slots of 256 KB (at most 64 MB whatever B), allocated here on the caller's stream.
    Its sums run in another order than ``coarse_score``'s, so the two agree to rounding, not bit for
    bit, on boxes both take.  CPU tensors take the same plain-torch statement as ``coarse_score``
    (which has no size bound of its own)."""
    return _coarse_score_op("wide", y, row_off, idx, yp, coef, iters, tau, out, idx_host, row_off_host, dtype,
                            row_scale)


def coarse_score_stream(y, row_off, idx, yp, coef, iters=10, tau=0.01, out=None, idx_host=None, row_off_host=None,
                        dtype=None, row_scale=None):
    """``coarse_score`` for every box the matcher takes, up to COARSE_STREAM_NMAX = 600 keypoints
    (fpm_coarse_score_stream): the same definition, arguments and host-side checks, with n0 and every
    selected n_g in [1, COARSE_STREAM_NMAX].  The kernel writes Kp to a scratch of min(B, 256) slots of
    min(n0, ngmax) x max(n0, ngmax) fp32 (ngmax: the largest selected n_g; at most 352 MiB whatever
    B), allocated here on the caller's stream, and streams the Sinkhorn from it: the first row step in
    place, the others on potentials.  It agrees with ``coarse_score`` and ``coarse_score_wide`` to
    rounding, not bit for bit, on boxes they take.  CPU tensors take the same plain-torch statement
    (which has no size bound of its own)."""
    return _coarse_score_op("stream", y, row_off, idx, yp, coef, iters, tau, out, idx_host, row_off_host, dtype,
                            row_scale)


def coarse_pairs(y, row_off, gidx, yq, qrow_off, qidx, coef, kernel="fused", iters=10, tau=0.01, out=None,
                 gidx_host=None, qidx_host=None, row_off_host=None, qrow_off_host=None, dtype=None, row_scale=None):
    """The coarse score over a pair list (fpm_coarse_pairs, _wide, _stream) -> (B,) fp32: pair b scores
    probe qidx[b] of the probe row store yq (sum n_q, 768) fp32 / qrow_off int64 [Q + 1] against entry
    gidx[b] of the index rows y / row_off (fp32, their bf16 copy: the _rows16 entry points, or float8_e4m3fn
    rows with their scales ``row_scale``: the _rows8 entry points) with
    coef[b], by the definition of ``coarse_score``.  ``kernel``: "fused" (boxes up to COARSE_NMAX),
    "wide" (COARSE_WIDE_NMAX) or "stream" (COARSE_STREAM_NMAX): the pair-list instantiation of that
    kernel, so score[b] is the same bits as ``coarse_score`` / ``_wide`` / ``_stream`` give for that
    probe, entry and coefficient row, whatever the order of the list and whatever else is in it.

    Checked on the host before anything is launched: dtypes, contiguity and devices, both index lists
    of one length and in range, every named n_q and n_g in [1, the kernel's bound], coef (B, 768)
    (``*_host``: host copies, so the checks need no device synchronisation).  CPU tensors take the
    plain-torch statement of ``coarse_score`` pair by pair, in ``dtype`` arithmetic."""
    op = "coarse_pairs"
    if kernel not in _COARSE_KERNELS:
        raise _lib.FpmError("%s: kernel must be one of %s" % (op, COARSE_KERNELS))
    _, _, bound, nmax, _ = _COARSE_KERNELS[kernel]
    _check_index_tensors(op, (("gidx", gidx, torch.int32), ("qidx", qidx, torch.int32),
                              ("row_off", row_off, torch.int64), ("qrow_off", qrow_off, torch.int64)))
    _check_coarse_rows(op, y, (("yq", yq), ("coef", coef)), row_scale)
    _check_on_device_of(op, y, (("row_off", row_off), ("gidx", gidx), ("yq", yq), ("qrow_off", qrow_off),
                                ("qidx", qidx), ("coef", coef), ("out", out)))
    G, Q, B = int(row_off.numel()) - 1, int(qrow_off.numel()) - 1, int(gidx.numel())
    if G < 1 or Q < 1:
        raise _lib.FpmError("%s: empty gallery or empty probe set" % op)
    if int(qidx.numel()) != B:
        raise _lib.FpmError("%s: gidx names %d pairs, qidx %d" % (op, B, int(qidx.numel())))
    _shape(coef, (B, 768), "%s coef" % op)
    gh, qh = _host_copy(gidx_host, gidx), _host_copy(qidx_host, qidx)
    oh, qoh = _host_copy(row_off_host, row_off), _host_copy(qrow_off_host, qrow_off)
    if gh.numel() != B or qh.numel() != B or oh.numel() != G + 1 or qoh.numel() != Q + 1:
        raise _lib.FpmError("%s: host copies of gidx / qidx / row_off / qrow_off do not match the device tensors" % op)
    for name, o, rows in (("row_off", oh, y), ("qrow_off", qoh, yq)):
        if not _offsets_rise(o, rows):
            raise _lib.FpmError("%s: %s must rise from 0 to the %d rows of its store" % (op, name, rows.shape[0]))
    nqmax = ngmax = 0
    if B:
        if int(gh.min()) < 0 or int(gh.max()) >= G:
            raise _lib.FpmError("%s: gidx value outside [0, %d)" % (op, G))
        if int(qh.min()) < 0 or int(qh.max()) >= Q:
            raise _lib.FpmError("%s: qidx value outside [0, %d)" % (op, Q))
        ng, nq = oh[gh + 1] - oh[gh], qoh[qh + 1] - qoh[qh]
        nqmax, ngmax = int(nq.max()), int(ng.max())
        for what, n in (("probe", nq), ("selected entry", ng)):
            if int(n.max()) > nmax or int(n.min()) < 1:
                raise _lib.FpmError("%s: a %s of %d keypoints; the %s coarse pass takes 1 to %s = %d"
                                    % (op, what, int(n.max()) if int(n.max()) > nmax else int(n.min()), kernel, bound,
                                       nmax))
    iters, tau = _check_iters_tau(op, iters, tau)
    if not y.is_cuda:
        dtype = _host_dtype(op, dtype)
        res = torch.empty(B, dtype=dtype)
        yh = y if row_scale is None else rows_dequant8(y, row_scale)
        for b in range(B):
            q = int(qh[b])
            res[b:b + 1] = _coarse_score_host(yh, oh, gh[b:b + 1], yq[int(qoh[q]):int(qoh[q + 1])], coef[b:b + 1], iters,
                                              tau, dtype)
        return _coarse_out(op, y, B, out, dtype, res)
    out = _coarse_out(op, y, B, out, dtype)
    if B:
        # the stream kernel's slots: the largest probe and the largest entry of the launch, from whichever pairs
        _coarse_call(kernel, True, y, (_p(y), *_scale_arg(row_scale), _p(row_off), _p(gidx), G, B, _p(yq), _p(qrow_off),
                                       _p(qidx), Q, _p(coef),
                                       iters, tau, _p(out)), B, nqmax, ngmax)
    return out


def edge_diff(x, src, dst):
    _dev(x, src, dst)
    E, D = src.numel(), x.shape[-1]
    out = torch.empty(E, D, device=x.device, dtype=torch.float32)
    _lib.call("fpm_edge_diff", _p(x), _p(src), _p(dst), E, D, _p(out), _stream(x))
    return out


def edge_diff_padded(x, src, dst, pair, row, nrows, cscale=None):
    """(nrows, D) zero-padded: out[row[e]] = (x[src[e]] - x[dst[e]]) * cscale[pair[e]]."""
    _dev(x, src, dst, pair, row)
    E, D = src.numel(), x.shape[-1]
    out = torch.zeros(nrows, D, device=x.device, dtype=torch.float32)
    _lib.call("fpm_edge_diff_padded", _p(x), _p(src), _p(dst), _p(pair), _p(row), _p(cscale), E, D, _p(out),
              _stream(x))
    return out


def gnn_layer(X, C, B, n1max, n2max, csr1, csr2, n1, n2, params, Xout, zbuf, vpart=None, cls_w=None, ord2=None):
    """``ord2``: optional (B, n2max) int32 block order of the graph-2 nodes (a schedule; same results)."""
    _dev(X, n1, n2, params, Xout, zbuf, vpart, cls_w, ord2)
    _shape(X, (B, C, n2max, n1max), "gnn_layer X")
    _shape(Xout, (B, 17, n2max, n1max), "gnn_layer Xout")
    _shape(zbuf, (B, n2max, n1max), "gnn_layer zbuf")
    _shape(vpart, (B, n2max, n1max), "gnn_layer vpart")
    _shape(ord2, (B, n2max), "gnn_layer ord2")
    _lib.call("fpm_kron_gnn_layer_fwd_ord", _p(X), C, B, n1max, n2max, ctypes.c_void_p(csr1[0]),
              ctypes.c_void_p(csr1[1]), ctypes.c_void_p(csr2[0]), ctypes.c_void_p(csr2[1]), _p(n1), _p(n2),
              _p(params), _p(Xout), _p(zbuf), _p(vpart), _p(cls_w), _p(ord2), _stream(X))


def gnn_resident_blocks(C, n1max):
    """Workgroups of the GNN layer's kernel for (C, n1max), under the current tuning, resident per CU
    (the runtime's occupancy query; no launch)."""
    nb = int(_lib.load().fpm_gnn_resident_blocks(int(C), int(n1max)))
    if nb < 0:
        raise _lib.FpmError(_lib.load().fpm_last_error().decode(errors="replace"))
    return nb


def node_classifier(X, B, n1max, n2max, w, b, out, vpart=None):
    _dev(X, w, b, out, vpart)
    _shape(X, (B, 17, n2max, n1max), "node_classifier X")
    _shape(out, (B, n1max, n2max), "node_classifier out")
    _shape(vpart, (B, n2max, n1max), "node_classifier vpart")
    _lib.call("fpm_node_classifier", _p(X), B, n1max, n2max, _p(w), _p(b), _p(vpart), _p(out), _stream(X))


def crossset_attn(cost, n2, Wv, mix1w, mix1b, mix2w, mix2b, out, split=False, stats=None):
    """``split``: out is (B * n1max, 768) bf16 [hi | lo | hi] rows (near-fp32 operand); ``stats``:
    optional (B * n1max, 16, 2) fp32 softmax (max, sum) per row and head (training)."""
    _dev(cost, n2, Wv, out)
    B, n1max, n2max = cost.shape
    _shape(out, (B * n1max, 768 if split else 256), "crossset_attn out")
    if split and out.dtype != torch.bfloat16:
        raise _lib.FpmError("crossset_attn: split rows are bf16")
    _shape(stats, (B * n1max, 16, 2), "crossset_attn stats")
    if n2max > 1 and cost.stride(2) != 1:
        raise _lib.FpmError("crossset_attn: cost rows must be contiguous (inner stride %d)" % cost.stride(2))
    _lib.call("fpm_crossset_attn_fwd", 2 if split else _code(out), _p(cost), cost.stride(0), cost.stride(1), B, n1max, n2max,
              _p(n2), _p(Wv), Wv.shape[1], _p(mix1w), _p(mix1b), _p(mix2w), _p(mix2b), _p(out), _p(stats),
              _stream(cost))


def instnorm(in1, B, P, Cn, w, b, in2=None, nvalid=None, onehot_bias=None, out_f=None, out_t=None, gmax=None,
             eps=1e-5, ldt=0):
    """``ldt`` > Cn: out_t rows are ldt wide and columns [Cn, ldt) are written as zeros."""
    code = _code(out_t) if out_t is not None else F32
    ref = in1 if in1 is not None else w
    _lib.call("fpm_instnorm", code, _p(in1), _p(in2), B, P, Cn, _p(nvalid), _p(onehot_bias), _p(w), _p(b),
              float(eps), _p(out_f), _p(out_t), int(ldt), _p(gmax), _stream(ref))


def gemm_norm_max(A, Bw, M, N, K, lda, ldb, bias, res, nw, nb, gmax, P=256, eps=1e-5):
    """AFA-U block tail fused (fpm_gemm_norm_max): gmax[b][n] = max over the pair's P rows of
    InstanceNorm(res + A Bw^T + bias) * nw + nb; bf16 A / Bw, P = 256 or 128 rows per pair (one or
    two pairs per 256-row tile)."""
    _dev(A, Bw, res, gmax)
    _lib.call("fpm_gemm_norm_max", _p(A), int(lda), _p(Bw), int(ldb), int(M), int(N), int(K), _p(bias), _p(res),
              int(res.stride(0)), _p(nw), _p(nb), float(eps), int(P), _p(gmax), _stream(A))
    return gmax


def gemm_norm_out(A, Bw, M, N, K, lda, ldb, bias, nw, nb, out_f, out_t=None, ldt=0, P=256, eps=1e-5):
    """AFA-U block head fused (fpm_gemm_norm_out): out_f = InstanceNorm over each pair's P rows of
    (A Bw^T + bias) * nw + nb, out_t its bf16 copy (row stride ldt, zero columns [N, ldt))."""
    _dev(A, Bw, out_f)
    _lib.call("fpm_gemm_norm_out", _p(A), int(lda), _p(Bw), int(ldb), int(M), int(N), int(K), _p(bias), _p(nw),
              _p(nb), float(eps), int(P), _p(out_f), int(out_f.stride(0)), _p(out_t),
              int(ldt or (out_t.stride(0) if out_t is not None else 0)), _stream(A))
    return out_f


def affinity(X1, X2, w, A_w, A_b, n1, n2, half=False, out=None):
    """InnerProductWithWeightsAffinity._forward for a batch of pairs (fpm_affinity_fwd,
    affinity_layer.py:11-19): X1 (B, n1max, d), X2 (B, n2max, d), w (B, kw) fp32 device tensors,
    A_w (d, kw), A_b (d,) -> K (B, n1max, n2max) = softplus((X1 o tanh(A_w w + A_b)) X2^T) - 0.5 on
    each pair's valid block (``half``: 0.5 * (...), the edge affinity), 0 elsewhere."""
    _dev(X1, X2, w, A_w, A_b, n1, n2)
    for t in (X1, X2, w, A_w, A_b):
        if t.dtype != torch.float32:
            raise _lib.FpmError("affinity: float32 operands expected")
    B, n1max, d = X1.shape
    n2max = X2.shape[1]
    kw = w.shape[1]
    _shape(X2, (B, n2max, d), "affinity X2")
    _shape(w, (B, kw), "affinity w")
    _shape(A_w, (d, kw), "affinity A_w")
    _shape(n1, (B,), "affinity n1")
    _shape(n2, (B,), "affinity n2")
    X1, X2, w, A_w = (t.contiguous() for t in (X1, X2, w, A_w))
    if out is None:
        out = torch.empty(B, n1max, n2max, device=X1.device, dtype=torch.float32)
    _shape(out, (B, n1max, n2max), "affinity out")
    nws = int(_lib.load().fpm_affinity_ws_floats(B, n1max, d))
    ws = torch.empty(max(nws, 1), device=X1.device, dtype=torch.float32)
    _lib.call("fpm_affinity_fwd", _p(X1), d, _p(X2), d, _p(w), kw, _p(A_w), _p(A_b), B, n1max, n2max, d,
              _p(n1.to(torch.int32)), _p(n2.to(torch.int32)), 1 if half else 0, _p(out), out.stride(1), _p(ws), nws,
              _stream(X1))
    return out


_RANGE = {"bad": None, "calls": 0}


def _range_every():
    import os
    return int(os.environ.get("FPM_LOSS_CHECK_EVERY", "1"))


def perm_loss_fwd(ds, gt, n1, n2, check_range=None):
    """PermutationLoss (src/loss_func.py:26-59) of device ds / gt (B, n1max, n2max views with unit
    column stride), n1 / n2 (B,) int32 device -> 0-d fp32 device tensor (fpm_perm_loss_fwd).  Each
    pair's block is clamped to the padded box like the reference's slice.

    Range check (the reference asserts 0 <= x <= 1 on both tensors, loss_func.py:42-47): entries of
    each pair's VALID block outside [0, 1] or NaN raise FpmError (the padding, which the reference's
    assert also covers, is not read: the device ds_mat is 0 there by construction).  The reference's
    assert reads the device on every call; here ``check_range`` (None: FPM_LOSS_CHECK_EVERY, default
    1) = 1 does the same, N > 1 accumulates the per-pair flags on the device and reads them every N-th
    call (the error names the calls since the last read), 0 / False skips the check."""
    _dev(ds, gt, n1, n2)
    B, n1max, n2max = ds.shape
    if ds.stride(2) != 1 or gt.stride(2) != 1 or tuple(gt.shape) != tuple(ds.shape):
        raise _lib.FpmError("perm_loss: ds / gt (B, n1max, n2max) with unit column stride expected")
    every = _range_every() if check_range is None else int(check_range)
    ws = torch.empty(B, device=ds.device, dtype=torch.float32)
    bad = torch.zeros(B, device=ds.device, dtype=torch.int32) if every > 0 else None
    out = torch.empty((), device=ds.device, dtype=torch.float32)
    _lib.call("fpm_perm_loss_fwd", _p(ds), ds.stride(0), ds.stride(1), _p(gt), gt.stride(0), gt.stride(1), _p(n1), _p(n2),
              B, n1max, n2max, _p(ws), _p(bad), _p(out), _stream(ds))
    if every <= 0:
        return out
    if every == 1:
        if int(bad.sum()):
            pairs = bad.nonzero().view(-1).tolist()
            raise _lib.FpmError("perm_loss: ds_mat / gt_perm_mat entries outside [0, 1] (or NaN) in pair(s) %s "
                                "(the reference asserts 0 <= x <= 1, loss_func.py:42-47)" % pairs[:8])
        return out
    acc = _RANGE["bad"]
    tot = bad.sum()
    _RANGE["bad"] = tot if acc is None or acc.device != tot.device else acc + tot
    _RANGE["calls"] += 1
    if _RANGE["calls"] >= every:
        n, calls = int(_RANGE["bad"]), _RANGE["calls"]
        _RANGE["bad"], _RANGE["calls"] = None, 0
        if n:
            raise _lib.FpmError("perm_loss: %d pair(s) with ds_mat / gt_perm_mat entries outside [0, 1] (or NaN) "
                                "in the last %d loss calls (the reference asserts 0 <= x <= 1, "
                                "loss_func.py:42-47)" % (n, calls))
    return out


def perm_loss_bwd(ds, gt, n1, n2, g):
    """d loss / d ds of perm_loss_fwd for the loss gradient ``g`` (0-d device tensor) -> contiguous
    (B, n1max, n2max) fp32."""
    _dev(ds, gt, n1, n2, g)
    B, n1max, n2max = ds.shape
    ws = torch.empty(1, device=ds.device, dtype=torch.float32)
    dds = torch.empty(B, n1max, n2max, device=ds.device, dtype=torch.float32)
    _lib.call("fpm_perm_loss_bwd", _p(ds), ds.stride(0), ds.stride(1), _p(gt), gt.stride(0), gt.stride(1), _p(n1), _p(n2),
              B, n1max, n2max, _p(g.float().contiguous()), _p(ws), _p(dds), _stream(ds))
    return dds


def gemm_x3out(A, Bw, M, N, K, Kp, epi=EPI_STORE, bias=None, out_t3=None, out_f=None, nw=None, nb=None, P=256,
               eps=1e-5):
    """C = epi(A Bw^T + bias) (bf16 A / Bw, fp32 accumulation) written as split bf16 rows
    out_t3 = [hi | lo | hi] (segment Kp, zero K padding; = split_bf16x3 of the fp32 C) and, if
    ``out_f`` is given, fp32 rows.  epi: EPI_STORE, EPI_RELU or EPI_NORM_OUT (instance norm over
    each pair's P = 256 or 128 rows, nw / nb) -- fpm_gemm_x3out.  Returns out_t3."""
    _dev(A, Bw, out_t3, out_f)
    for t, w in ((A, "A"), (Bw, "B")):
        if t.dtype != torch.bfloat16 or t.dim() != 2 or t.stride(1) != 1:
            raise _lib.FpmError("gemm_x3out: %s must be (rows, K) bf16 rows with unit stride" % w)
    if A.shape[0] < M or A.shape[1] < K or Bw.shape[0] != N or Bw.shape[1] < K:
        raise _lib.FpmError("gemm_x3out: operand shapes %s x %s do not cover M=%d N=%d K=%d"
                            % (tuple(A.shape), tuple(Bw.shape), M, N, K))
    if out_t3 is None:
        out_t3 = torch.empty(M, 3 * Kp, device=A.device, dtype=torch.bfloat16)
    if out_t3.dtype != torch.bfloat16 or out_t3.shape[0] != M or out_t3.stride(1) != 1 or out_t3.shape[1] < 3 * Kp:
        raise _lib.FpmError("gemm_x3out: out_t3 must be (M, >= 3 Kp) bf16")
    if out_f is not None and (out_f.dtype != torch.float32 or out_f.shape[0] != M or out_f.shape[1] < N):
        raise _lib.FpmError("gemm_x3out: out_f must be (M, >= N) float32")
    _lib.call("fpm_gemm_x3out", _p(A), int(A.stride(0)), _p(Bw), int(Bw.stride(0)), int(M), int(N), int(K), int(epi),
              _p(bias), _p(nw), _p(nb), float(eps), int(P), _p(out_f), int(out_f.stride(0)) if out_f is not None else 0,
              _p(out_t3), int(out_t3.stride(0)), int(Kp), _stream(A))
    return out_t3


def afau_head(gr, gc, B, E, r0w, r0b, r2w, r2b, c0w, c0b, c2w, c2b, ks):
    _lib.call("fpm_afau_head", _p(gr), _p(gc), B, E, _p(r0w), _p(r0b), _p(r2w), _p(r2b), _p(c0w), _p(c0b),
              _p(c2w), _p(c2b), _p(ks), _stream(gr))


# ---- fp64 k chain (csrc/precise.hip): Kp -> GNN layers -> readout -> final Sinkhorn -> AFA-U -------
def _f64(*ts):
    for t in ts:
        if t is not None and t.dtype != torch.float64:
            raise _lib.FpmError("fp64 k-chain op: float64 tensor expected, got %s" % t.dtype)


def gnn_layer_f64(X, C, B, n1max, n2max, csr1, csr2, n1, n2, params, Xout, zbuf):
    """PYGNNLayer in fp64: X (B, C, n2max, n1max) fp32 Kp for C = 1, the fp64 state for C = 17 ->
    Xout[:, 0:16] (fp64) and zbuf (B, n2max, n1max) fp64 (fpm_kron_gnn_layer_fwd_f64)."""
    _dev(X, n1, n2, params, Xout, zbuf)
    _shape(X, (B, C, n2max, n1max), "gnn_layer_f64 X")
    _shape(Xout, (B, 17, n2max, n1max), "gnn_layer_f64 Xout")
    _shape(zbuf, (B, n2max, n1max), "gnn_layer_f64 zbuf")
    _f64(Xout, zbuf)
    if not (X.is_contiguous() and Xout.is_contiguous() and zbuf.is_contiguous()):
        raise _lib.FpmError("gnn_layer_f64: contiguous tensors expected")
    x64 = X.dtype == torch.float64
    if x64 != (C == 17) or (not x64 and X.dtype != torch.float32):
        raise _lib.FpmError("gnn_layer_f64: layer 0 reads fp32 Kp (C = 1), later layers the fp64 state (C = 17)")
    _lib.call("fpm_kron_gnn_layer_fwd_f64", _p(X), int(x64), C, B, n1max, n2max, ctypes.c_void_p(csr1[0]),
              ctypes.c_void_p(csr1[1]), ctypes.c_void_p(csr2[0]), ctypes.c_void_p(csr2[1]), _p(n1), _p(n2),
              _p(params), _p(Xout), _p(zbuf), _stream(X))


def sinkhorn_f64(s, n1, n2, iters, tau, dummy_row=True, out=None, out32=None):
    """pygm log Sinkhorn in fp64 on each pair's valid block of the (n1max, n2max) box: ``s`` any
    strided fp32 / fp64 3-D view, ``out`` an fp64 view (allocated when None and ``out32`` is None),
    ``out32`` an optional fp32 copy.  Boxes up to 128 x 128."""
    _dev(s, n1, n2, out, out32)
    B, n1max, n2max = s.shape
    if out is None and out32 is None:
        out = torch.empty(B, n1max, n2max, device=s.device, dtype=torch.float64)
    _shape(out, (B, n1max, n2max), "sinkhorn_f64 out")
    _shape(out32, (B, n1max, n2max), "sinkhorn_f64 out32")
    _shape(n1, (B,), "sinkhorn_f64 n1")
    _shape(n2, (B,), "sinkhorn_f64 n2")
    _f64(out)
    if out32 is not None and out32.dtype != torch.float32:
        raise _lib.FpmError("sinkhorn_f64: out32 must be float32")
    if s.dtype not in (torch.float32, torch.float64):
        raise _lib.FpmError("sinkhorn_f64: s must be float32 or float64")
    st = lambda t: (t.stride(0), t.stride(1), t.stride(2)) if t is not None else (0, 0, 0)
    _lib.call("fpm_sinkhorn_log_fwd_f64", _p(s), int(s.dtype == torch.float64), *st(s), _p(out), *st(out), _p(out32),
              *st(out32), _p(n1), _p(n2), B, n1max, n2max, int(iters), float(tau), int(bool(dummy_row)), _stream(s))
    return out


def node_classifier_f64(X, B, n1max, n2max, w, b, s64, s32=None):
    """s = classifier(emb) (ngm.py:368-369) from the fp64 state: s64 (B, n1max, n2max) fp64 and
    optionally its fp32 copy."""
    _dev(X, w, b, s64, s32)
    _shape(X, (B, 17, n2max, n1max), "node_classifier_f64 X")
    _shape(s64, (B, n1max, n2max), "node_classifier_f64 s64")
    _shape(s32, (B, n1max, n2max), "node_classifier_f64 s32")
    _f64(X, s64)
    for t in (X, s64, s32):
        if t is not None and not t.is_contiguous():
            raise _lib.FpmError("node_classifier_f64: contiguous tensors expected")
    _lib.call("fpm_node_classifier_f64", _p(X), B, n1max, n2max, _p(w), _p(b), _p(s64), _p(s32), _stream(X))


def crossset_attn_row_f64(cost, n2, Wv, mix1w, mix1b, mix2w, mix2b, out):
    """The AFA-U row block's cross-set attention (R0 = 0) in fp64: cost (B, n1max, n2max) fp64 with
    unit column stride -> out (B * n1max, 256) fp64."""
    _dev(cost, n2, Wv, out)
    _f64(cost, Wv, mix1w, mix1b, mix2w, mix2b, out)
    B, n1max, n2max = cost.shape
    _shape(out, (B * n1max, 256), "crossset_attn_row_f64 out")
    if cost.stride(2) != 1 or not Wv.is_contiguous() or not out.is_contiguous():
        raise _lib.FpmError("crossset_attn_row_f64: unit-stride cost rows, contiguous Wv / out expected")
    _lib.call("fpm_crossset_attn_row_f64", _p(cost), cost.stride(0), cost.stride(1), B, n1max, n2max, _p(n2), _p(Wv),
              Wv.shape[1], _p(mix1w), _p(mix1b), _p(mix2w), _p(mix2b), _p(out), _stream(cost))


def gemm_f64(A, W, bias=None, relu=False, out=None):
    """out = act(A @ W^T + bias) in fp64 (fpm_gemm_f64): A (M, K), W (N, K)."""
    _dev(A, W, bias, out)
    _f64(A, W, bias, out)
    M, K = A.shape
    N = W.shape[0]
    if W.shape[1] != K or A.stride(1) != 1 or W.stride(1) != 1:
        raise _lib.FpmError("gemm_f64: A (M, K), W (N, K) with unit column stride expected")
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=torch.float64)
    _shape(out, (M, N), "gemm_f64 out")
    _lib.call("fpm_gemm_f64", _p(A), A.stride(0), _p(W), W.stride(0), _p(bias), _p(out), out.stride(0), M, N, K,
              int(bool(relu)), _stream(A))
    return out


def instnorm_f64(in1, B, P, Cn, w, b, in2=None, nvalid=None, onehot_bias=None, out=None, gmax=None, eps=1e-5):
    """AddAndInstanceNormalization (afau.py:154-176) in fp64 over each pair's P rows of Cn channels:
    x = in1 (+ in2), or the col block's one-hot + bias; out (B * P, Cn) and/or gmax (B, Cn)."""
    ref = in1 if in1 is not None else w
    _dev(ref, in2, nvalid, onehot_bias, w, b, out, gmax)
    _f64(in1, in2, onehot_bias, w, b, out, gmax)
    for t in (in1, in2, out):
        _shape(t, (B * P, Cn), "instnorm_f64 rows")
    _shape(gmax, (B, Cn), "instnorm_f64 gmax")
    _lib.call("fpm_instnorm_f64", _p(in1), _p(in2), B, P, Cn, _p(nvalid), _p(onehot_bias), _p(w), _p(b), float(eps),
              _p(out), _p(gmax), _stream(ref))


def afau_head_f64(gr, gc, cidx, B, E, r0w, r0b, r2w, r2b, c0w, c0b, c2w, c2b, ks):
    """ks = sigmoid((final_row(gr) + final_col(gc[cidx])) / 2) from fp64 pooled rows -> ks fp32."""
    _dev(gr, gc, cidx, ks)
    _f64(gr, gc, r0w, r0b, r2w, r2b, c0w, c0b, c2w, c2b)
    _shape(gr, (B, E), "afau_head_f64 gr")
    _shape(ks, (B,), "afau_head_f64 ks")
    if cidx is not None and (cidx.dtype != torch.int32 or tuple(cidx.shape) != (B,)):
        raise _lib.FpmError("afau_head_f64: cidx must be int32 (B,)")
    _lib.call("fpm_afau_head_f64", _p(gr), _p(gc), _p(cidx), B, E, _p(r0w), _p(r0b), _p(r2w), _p(r2b), _p(c0w),
              _p(c0b), _p(c2w), _p(c2b), _p(ks), _stream(gr))


def soft_topk_f64(ss, n1, n2, k, iters=10, tau=0.01, out=None, steps=None, out_host=None):
    """soft_topk(..., return_prob=True)[1] in fp64 from the fp64 ss (unit column stride) -> ds_mat
    fp32 (B, n1max, n2max); ``steps``: (B,) int32 steps taken incl. the while loop; ``out_host``: a
    pinned host copy written by the kernel too."""
    _dev(ss, n1, n2, k, out, steps)
    _f64(ss)
    B, n1max, n2max = ss.shape
    if ss.stride(2) != 1:
        raise _lib.FpmError("soft_topk_f64: ss rows with unit column stride expected")
    if out is None:
        out = torch.empty(B, n1max, n2max, device=ss.device, dtype=torch.float32)
    _shape(out, (B, n1max, n2max), "soft_topk_f64 out")
    for t, w in ((n1, "n1"), (n2, "n2"), (k, "k"), (steps, "steps")):
        _shape(t, (B,), "soft_topk_f64 " + w)
    if out.stride(2) != 1 or (out_host is not None and (out_host.is_cuda or not out_host.is_pinned()
                                                       or tuple(out_host.shape) != (B, n1max, n2max))):
        raise _lib.FpmError("soft_topk_f64: out with unit column stride, out_host pinned (B, n1max, n2max)")
    ws = torch.empty(2 * B * n1max * n2max, device=ss.device, dtype=torch.float64)
    _lib.call("fpm_soft_topk_fwd_f64", _p(ss), ss.stride(0), ss.stride(1), _p(n1), _p(n2), _p(k), B, n1max, n2max,
              int(iters), float(tau), _p(ws), ws.numel(), _p(out), out.stride(0), out.stride(1), _p(steps),
              _p(out_host), out_host.stride(0) if out_host is not None else 0,
              out_host.stride(1) if out_host is not None else 0, _stream(ss))
    return out


def match_cls(s, perm, w1, b1, bn1_sc, bn1_sh, w2, b2, bn2_sc, bn2_sh, fcw, fcb, logits=None, prob=None, dtype=F32):
    _dev(s, perm)
    if not (s.is_contiguous() and perm.is_contiguous()):
        raise _lib.FpmError("match_cls: s and perm must be contiguous")
    B, H, W = s.shape
    nws = _lib.load().fpm_match_cls_ws_floats(B, H, W)
    ws = torch.empty(max(int(nws), 1), device=s.device, dtype=torch.float32)
    logits = logits if logits is not None else torch.empty(B, device=s.device, dtype=torch.float32)
    prob = prob if prob is not None else torch.empty(B, device=s.device, dtype=torch.float32)
    _lib.call("fpm_match_cls_fwd", int(dtype), _p(s), _p(perm), B, H, W, _p(w1), _p(b1), _p(bn1_sc), _p(bn1_sh), _p(w2), _p(b2),
              _p(bn2_sc), _p(bn2_sh), _p(fcw), _p(fcb), _p(ws), _p(logits), _p(prob), _stream(s))
    return logits, prob


def feature_align(nodes, edges, P, n, nmax=None, ori_size=(320.0, 240.0), out=None, wglob=None, keep_ws=False):
    """Normalise both CNN maps over channels, bilinear-gather them at the keypoints
    (utils/feature_align.py) and concatenate -> X (B*nmax, C_n + C_e) fp32 with zero padding rows;
    also the global max-pooled edge feature (B, C_e).  Maps may be NCHW or channels_last.
    ``keep_ws``: also return the workspace (pixel norms) for feature_align_bwd."""
    _dev(nodes, edges, P, n)
    for t in (nodes, edges, P):
        if t.dtype != torch.float32:
            raise _lib.FpmError("feature_align: float32 maps and keypoints expected")
    if nodes.dim() != 4 or edges.dim() != 4 or P.dim() != 3 or P.shape[-1] != 2:
        raise _lib.FpmError("feature_align: maps (B, C, H, W) and keypoints (B, nmax, 2) expected")
    B = int(nodes.shape[0])
    nmax = int(P.shape[1]) if nmax is None else int(nmax)
    if int(P.shape[0]) != B or int(P.shape[1]) != nmax or n.numel() != B or n.dtype != torch.int32:
        raise _lib.FpmError("feature_align: P must be (B, nmax, 2) and n (B,) int32")
    P = P.contiguous()
    C = int(nodes.shape[1]) + int(edges.shape[1])
    if out is None:
        out = torch.empty(B * nmax, C, dtype=torch.float32, device=nodes.device)
    if wglob is None:
        wglob = torch.empty(B, int(edges.shape[1]), dtype=torch.float32, device=nodes.device)
    arr = lambda v: ctypes.cast((ctypes.c_long * 4)(*[int(x) for x in v]), ctypes.c_void_p)
    ns_, nst, es_, est = arr(nodes.shape), arr(nodes.stride()), arr(edges.shape), arr(edges.stride())
    lib = _lib.load()
    ws = torch.empty(int(lib.fpm_feature_align_ws_floats(ns_, es_)), dtype=torch.float32, device=nodes.device)
    _lib.call("fpm_feature_align_fwd", _p(nodes), ns_, nst, _p(edges), es_, est, _p(P), _p(n), nmax,
              float(ori_size[0]), float(ori_size[1]), _p(ws), _p(out), int(out.stride(0)), _p(wglob), _stream(nodes))
    return (out, wglob, ws) if keep_ws else (out, wglob)


def feature_align_bwd(nodes, edges, P, n, ws, dX, dwglob=None, ori_size=(320.0, 240.0)):
    """Backward of feature_align: gradients of X rows (and of the global feature) -> gradients of
    the raw maps (dnodes, dedges), allocated with the maps' memory formats."""
    _dev(nodes, edges, P, n, ws, dX)
    B = int(nodes.shape[0])
    nmax = int(P.shape[1])
    Cn, Ce = int(nodes.shape[1]), int(edges.shape[1])
    if dX.dtype != torch.float32 or dX.dim() != 2 or dX.shape[0] != B * nmax or dX.shape[1] < Cn + Ce or dX.stride(1) != 1:
        raise _lib.FpmError("feature_align_bwd: dX must be (B*nmax, >= C_n + C_e) float32 rows")
    if dwglob is not None:
        _shape(dwglob, (B, Ce), "feature_align_bwd dwglob")
        dwglob = dwglob.contiguous().float()
    P = P.contiguous()
    fmt = lambda t: torch.channels_last if t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous() \
        else torch.contiguous_format
    dn = torch.empty_like(nodes, memory_format=fmt(nodes))
    de = torch.empty_like(edges, memory_format=fmt(edges))
    arr = lambda v: ctypes.cast((ctypes.c_long * 4)(*[int(x) for x in v]), ctypes.c_void_p)
    _lib.call("fpm_feature_align_bwd", _p(nodes), arr(nodes.shape), arr(nodes.stride()), _p(edges), arr(edges.shape),
              arr(edges.stride()), _p(P), _p(n), nmax, float(ori_size[0]), float(ori_size[1]), _p(ws), _p(dX),
              int(dX.stride(0)), _p(dwglob), _p(dn), arr(dn.stride()), _p(de), arr(de.stride()), _stream(nodes))
    return dn, de


def lsa_batch_device(s, n1, n2, assign=None, status=None):
    """Device LSA (maximise s) over a (B, n1max, n2max) float32 view with unit column stride ->
    (assign (B, n1max) int32, status (B,) int32); bit-identical to ``lsa_batch_host``.  Asynchronous:
    check ``status`` (0 ok, 1 infeasible, 2 NaN/-inf) after synchronising."""
    _dev(s, n1, n2)
    if s.dtype != torch.float32 or s.dim() != 3 or s.stride(2) != 1:
        raise _lib.FpmError("lsa_batch_device: (B, n1max, n2max) float32 with unit column stride expected")
    B, n1max, n2max = s.shape
    if assign is None:
        assign = torch.empty(B, n1max, dtype=torch.int32, device=s.device)
    if status is None:
        status = torch.empty(B, dtype=torch.int32, device=s.device)
    _lib.call("fpm_lsa_batch_device", _p(s), int(s.stride(0)), int(s.stride(1)), _p(n1), _p(n2), B, n1max, n2max,
              _p(assign), _p(status), _stream(s))
    return assign, status


def _assign_out(out, B, n1max):
    if out is None:
        return torch.empty(B, n1max, dtype=torch.int32)
    if out.is_cuda or out.dtype != torch.int32 or tuple(out.shape) != (B, n1max) or not out.is_contiguous():
        raise _lib.FpmError("lsa: out must be a contiguous host (B, n1max) int32 tensor")
    return out


def lsa_batch_host(s_host, n1_host, n2_host, nthreads=1, b0=0, out=None):
    """Host LSA (maximise s) over a pinned/CPU float32 (B, n1max, n2max) tensor -> (B, n1max) int32.
    ``b0``: the batch's first pair index in the caller's batch (error messages report b0 + pair);
    ``out``: optional host (B, n1max) int32 result tensor (pinned: its H2D copy stays asynchronous)."""
    if s_host.is_cuda:
        raise _lib.FpmError("lsa_batch_host expects host memory")
    s_host = s_host.contiguous()
    B, n1max, n2max = s_host.shape
    n1c = n1_host.to(torch.int32).contiguous()
    n2c = n2_host.to(torch.int32).contiguous()
    out = _assign_out(out, B, n1max)
    rc = _lib.load().fpm_lsa_batch_host(_p(s_host), n1max * n2max, n2max, _p(n1c), _p(n2c), B, n1max, _p(out),
                                        int(nthreads))
    if rc != 0:
        raise _lib.FpmError("hungarian: pair %d is infeasible or has NaN/-inf costs" % (b0 + rc - 1))
    return out


class LsaTicket:
    """A batch queued on the host LSA workers (``lsa_submit``); holds its tensors until waited.
    Every ticket must be waited (``lsa_wait``) before its tensors are dropped: the workers read the
    cost rows and write the assignment until then (``lsa_drain`` waits for a set of tickets)."""

    def __init__(self, ticket, keep, out, b0=0):
        self.ticket, self._keep, self.out, self.b0 = ticket, keep, out, b0
        self.seconds = 0.0
        self.waited = False


def lsa_submit(s_host, n1_host, n2_host, nthreads=1, b0=0, out=None):
    """Asynchronous ``lsa_batch_host``: queue the batch on the persistent LSA workers (pairs of
    successive batches are served first-in first-out) and return a ticket for ``lsa_wait``.
    ``b0``: the batch's first pair index in the caller's batch (error messages report b0 + pair)."""
    if s_host.is_cuda:
        raise _lib.FpmError("lsa_submit expects host memory")
    s_host = s_host.contiguous()
    B, n1max, n2max = s_host.shape
    n1c = n1_host.to(torch.int32).contiguous()
    n2c = n2_host.to(torch.int32).contiguous()
    out = _assign_out(out, B, n1max)
    t = _lib.load().fpm_lsa_submit(_p(s_host), n1max * n2max, n2max, _p(n1c), _p(n2c), B, n1max, _p(out),
                                   int(nthreads))
    return LsaTicket(t, (s_host, n1c, n2c), out, b0)


def lsa_wait(tk, block=True):
    """The assignment of a ``lsa_submit`` batch ((B, n1max) int32), or None if ``block`` is False
    and it is still running.  ``tk.seconds``: the batch's span on the workers."""
    sec = ctypes.c_double(0.0)
    rc = _lib.load().fpm_lsa_wait(tk.ticket, 1 if block else 0, ctypes.byref(sec))
    if rc == -2:
        return None
    if rc == -1:
        raise _lib.FpmError("lsa_wait: unknown or already waited ticket")
    tk.waited = True
    tk.seconds = sec.value
    if rc != 0:
        raise _lib.FpmError("hungarian: pair %d is infeasible or has NaN/-inf costs" % (tk.b0 + rc - 1))
    return tk.out


def lsa_drain(tickets):
    """Block until every not-yet-waited ticket's batch is done (results and errors discarded): the
    cleanup path of a forward that stops early, so no worker still reads or writes its buffers."""
    for tk in tickets:
        if not tk.waited:
            try:
                lsa_wait(tk)
            except _lib.FpmError:
                pass


# ---- training backward -----------------------------------------------------
def sinkhorn_bwd(s, dp, ds, n1, n2, iters, tau, dummy_row, ws):
    """d/ds of ``sinkhorn`` given dp = d/d(out); s, dp: strided (B, n1max, n2max) views; ds contiguous."""
    _dev(s, dp, ds, n1, n2, ws)
    B, n1max, n2max = s.shape
    if tuple(dp.shape) != (B, n1max, n2max) or not ds.is_contiguous() or tuple(ds.shape) != (B, n1max, n2max):
        raise _lib.FpmError("sinkhorn_bwd: shape mismatch")
    _lib.call("fpm_sinkhorn_log_bwd", _p(s), s.stride(0), s.stride(1), s.stride(2), _p(dp), dp.stride(0),
              dp.stride(1), dp.stride(2), _p(ds), _p(n1), _p(n2), B, n1max, n2max, int(iters), float(tau),
              int(bool(dummy_row)), _p(ws), ws.numel(), _stream(s))
    return ds


def soft_topk_bwd(ss, n1, n2, k, steps, tau, dds):
    """d/dss of ``soft_topk`` (k and steps as used / returned by the forward) -> (B, n1max, n2max)."""
    _dev(ss, n1, n2, k, steps, dds)
    B, n1max, n2max = ss.shape
    if ss.stride(2) != 1 or dds.stride(2) != 1 or tuple(dds.shape) != (B, n1max, n2max):
        raise _lib.FpmError("soft_topk_bwd: (B, n1max, n2max) views with unit column stride expected")
    lib = _lib.load()
    ws = torch.empty(max(int(lib.fpm_soft_topk_bwd_ws_floats(B, n1max, n2max)), 1), device=ss.device,
                     dtype=torch.float32)
    status = torch.zeros(B, device=ss.device, dtype=torch.int32)
    dss = torch.empty(B, n1max, n2max, device=ss.device, dtype=torch.float32)
    _lib.call("fpm_soft_topk_bwd", _p(ss), ss.stride(0), ss.stride(1), _p(n1), _p(n2), _p(k), _p(steps), B, n1max,
              n2max, float(tau), _p(dds), dds.stride(0), dds.stride(1), _p(dss), _p(ws), ws.numel(), _p(status),
              _stream(ss))
    if int(status.sum()):
        raise _lib.FpmError("soft_topk_bwd: forward ran more steps than the backward replay holds")
    return dss


def spline_plan_rows(plan, E, num_nodes):
    """(arows, cell_off) int32 views into a plan: product row -> source node, per-cell row ranges."""
    a, c = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.call("fpm_spline_plan_rows", _p(plan), E, num_nodes, ctypes.byref(a), ctypes.byref(c))
    base = plan.data_ptr()
    oa, oc = a.value - base, c.value - base
    arows = plan[oa:].view(torch.int32)
    cell_off = plan[oc:oc + 4 * 27].view(torch.int32)
    return arows, cell_off


def spline_plan_edges(plan, E, num_nodes):
    """(csr_e (E,) int32, rows4 (E, 4) int32, basis4 (E, 4) float32) views into a plan: per CSR slot
    of the in-edge lists, the edge id, its 4 product rows and its 4 basis weights (corner order)."""
    a, r, b = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    _lib.call("fpm_spline_plan_edges", _p(plan), E, num_nodes, ctypes.byref(a), ctypes.byref(r), ctypes.byref(b))
    base = plan.data_ptr()
    oa, orr, ob = a.value - base, r.value - base, b.value - base
    csr_e = plan[oa:oa + 4 * E].view(torch.int32)
    rows4 = plan[orr:orr + 16 * E].view(torch.int32).view(E, 4)
    basis4 = plan[ob:ob + 16 * E].view(torch.float32).view(E, 4)
    return csr_e, rows4, basis4


def spline_conv_bwd_data(x_op, plan, E, num_nodes, nmax, nvalid, Wb, y_ws, mode, gout, hout, dY, dY_op, dXrows, dX,
                         accumulate=False, rplan=None, argmax=None):
    """Input gradient of one SplineConv layer (see include/fpm.h); fills dY (product-row grads).
    rplan (plan of the reversed edges) + argmax (from spline_conv(..., argmax=)): the atomic-free
    scatter form."""
    _dev(plan, nvalid, Wb, y_ws, gout, dY, dXrows, dX)
    code = _code(x_op)
    if _code(Wb) != code or tuple(Wb.shape) != (26, 768, 768):
        raise _lib.FpmError("spline_conv_bwd: Wb must be (26, 768, 768) in the operand dtype")
    if mode == 0 and hout is None:
        raise _lib.FpmError("spline_conv_bwd: mode 0 needs the layer output")
    if (rplan is None) != (argmax is None):
        raise _lib.FpmError("spline_conv_bwd: rplan and argmax go together")
    _lib.call("fpm_spline_conv_bwd_data_scatter", code, _p(plan), _p(rplan), _p(argmax), E, num_nodes, nmax,
              _p(nvalid), _p(Wb), _p(y_ws), int(mode), _p(gout), _p(hout), _p(dY), _p(dY_op), _p(dXrows), _p(dX),
              int(bool(accumulate)), _stream(gout))


def kron_agg(X, C, B, n1max, n2max, tcsr1, tcsr2, q1, q2, n1, n2, adjoint, out, accumulate=False):
    """Factorised Kronecker SAGE-mean aggregation (adjoint=False: forward agg over the in-edge CSRs
    tcsr*; adjoint=True: its transpose over the out-edge CSRs).  q1/q2: in-edge CSR pointers.
    ``accumulate``: out += result."""
    _dev(X, n1, n2, out)
    _lib.call("fpm_kron_agg", _p(X), int(C), int(B), int(n1max), int(n2max), ctypes.c_void_p(tcsr1[0]),
              ctypes.c_void_p(tcsr1[1]), ctypes.c_void_p(tcsr2[0]), ctypes.c_void_p(tcsr2[1]), ctypes.c_void_p(q1),
              ctypes.c_void_p(q2), _p(n1), _p(n2), int(bool(adjoint)) | (2 if accumulate else 0), _p(out), _stream(X))
    return out


def gnn_layer_bwd_point(X, C, B, n1max, n2max, dXn, dz, params, dX, dagg, V):
    """Per-position PYGNNLayer backward (node MLPs + classifier): dX (direct part), dagg, and
    V = [dx1 | dh1 | dm | h1] (B, 64, N) for the weight-gradient reductions."""
    _dev(X, dXn, dz, params, dX, dagg, V)
    for t in (X, dXn, dz, dX, dagg, V):
        if not t.is_contiguous():
            raise _lib.FpmError("gnn_layer_bwd_point: contiguous tensors expected")
    _lib.call("fpm_kron_gnn_layer_bwd_point", _p(X), int(C), int(B), int(n1max), int(n2max), _p(dXn), _p(dz),
              _p(params), _p(dX), _p(dagg), _p(V), _stream(X))


def _counts(n, B, full, dev):
    """nrows / ncols as the kernels take them: int32 on ``dev``; None -> the unpadded size."""
    if n is None:
        return torch.full((B,), int(full), dtype=torch.int32, device=dev)
    return torch.as_tensor(n).reshape(-1).to(device=dev, dtype=torch.int32)


class Sinkhorn(torch.nn.Module):
    """``Sinkhorn(max_iter=10, tau=1., epsilon=1e-4, log_forward=True, batched_operation=False)``
    (``src/model/sinkhorn.py:7-87``), whose ``forward_log`` is ``pygmtools.sinkhorn``: log-domain
    alternating row / column normalisation of ``s / tau`` on each pair's valid block, dummy rows
    when asked, pairs with n1 > n2 run transposed.  Differentiable (``fpm_sinkhorn_log_bwd``).
    ``epsilon`` and ``batched_operation`` do not change the log-domain result and are accepted
    for signature parity."""

    def __init__(self, max_iter=10, tau=1., epsilon=1e-4, log_forward=True, batched_operation=False):
        super().__init__()
        if not log_forward:
            # forward_ori is deprecated in the reference (sinkhorn.py:53-54); only the log form is built
            raise NotImplementedError("Sinkhorn(log_forward=False) is not built: use the log-domain forward")
        self.max_iter, self.tau, self.epsilon = max_iter, tau, epsilon
        self.log_forward, self.batched_operation = log_forward, batched_operation

    def forward(self, s, nrows=None, ncols=None, dummy_row=False):
        return self.forward_log(s, nrows, ncols, dummy_row)

    def forward_log(self, s, nrows=None, ncols=None, dummy_row=False):
        _dev(s)
        matrix_input = s.dim() == 2
        if matrix_input:
            s = s.unsqueeze(0)
        if s.dim() != 3:
            raise ValueError("input data shape not understood: %s" % (tuple(s.shape),))
        B, n1max, n2max = s.shape
        n1 = _counts(nrows, B, n1max, s.device)
        n2 = _counts(ncols, B, n2max, s.device)
        sf = s.float()
        if sf.requires_grad and torch.is_grad_enabled():
            from .train import SinkhornFn
            out = SinkhornFn.apply(sf, n1, n2, int(self.max_iter), float(self.tau), bool(dummy_row))
        else:
            out = sinkhorn(sf.detach(), n1, n2, int(self.max_iter), float(self.tau), bool(dummy_row))
        out = out.to(s.dtype)
        return out.squeeze(0) if matrix_input else out


def greedy_perm(x, top_indices, ks):
    """``greedy_perm(x, top_indices, ks)`` (``src/model/soft_topk.py:56-77``): walk each pair's
    candidate order and accept (idx // n2max, idx % n2max) while its row and column of ``x`` still
    sum to < 1, until ``round(ks[b])`` (half-to-even) are accepted.  ``x`` is updated in place and
    returned (fpm_greedy_perm)."""
    _dev(x, top_indices)
    if x.dim() != 3 or x.dtype != torch.float32 or x.stride(2) != 1:
        raise _lib.FpmError("greedy_perm: x must be a (b, n1, n2) float32 tensor with unit column stride")
    B, n1max, n2max = x.shape
    top = top_indices.reshape(B, -1).to(torch.int64).contiguous()
    k = torch.as_tensor(ks).reshape(-1).to(device=x.device, dtype=torch.float32).contiguous()
    if k.numel() != B:
        raise _lib.FpmError("greedy_perm: ks must hold one count per pair")
    _lib.call("fpm_greedy_perm", _p(top), top.stride(0), int(top.shape[1]), _p(k), B, n1max, n2max, _p(x),
              x.stride(0), x.stride(1), _stream(x))
    return x


def soft_topk(scores, ks, max_iter=10, tau=1., nrows=None, ncols=None, return_prob=False):
    """``soft_topk(scores, ks, max_iter, tau, nrows, ncols, return_prob)``
    (``src/model/soft_topk.py:8-53``): the 2-column marginal Sinkhorn incl. ``Sinkhorn_m``'s
    data-dependent continuation (fpm_soft_topk_fwd), then the reference's own hard output:
    candidates in descending order of P(top-k) over the pair's flattened valid block
    (q = i * n2 + j, padded to max(nrows) * max(ncols) with zeros), decoded with the box width
    like the reference's greedy_perm.  Ties keep ascending flat index (the reference's argsort is
    unstable, quirk A.10(v)).  Returns x, or (x, soft matrix) with ``return_prob``.  The soft
    matrix is differentiable in ``scores`` (fpm_soft_topk_bwd)."""
    _dev(scores)
    B, n1max, n2max = scores.shape
    n1 = _counts(nrows, B, n1max, scores.device)
    n2 = _counts(ncols, B, n2max, scores.device)
    k = torch.as_tensor(ks).reshape(-1).to(device=scores.device, dtype=torch.float32)
    sf = scores.float()
    if sf.requires_grad and torch.is_grad_enabled():
        from .train import SoftTopkFn
        out_s = SoftTopkFn.apply(sf, k, n1, n2, int(max_iter), float(tau))
    else:
        out_s = soft_topk_fwd(sf.detach().contiguous(), n1, n2, k.contiguous(), int(max_iter), float(tau))
    # the reference's output[:, :, 1]: (b, max(nrows) * max(ncols)), pair b's block row-major first
    L = int(n1.max()) * int(n2.max())
    q = torch.arange(L, device=scores.device)
    n2l = n2.long()[:, None]
    valid = q[None, :] < (n1.long() * n2.long())[:, None]
    flat = out_s.detach()[torch.arange(B, device=scores.device)[:, None],
                          torch.where(valid, q[None, :] // n2l, 0), torch.where(valid, q[None, :] % n2l, 0)]
    flat = torch.where(valid, flat, torch.zeros((), device=scores.device))
    top = torch.argsort(flat, dim=-1, descending=True, stable=True)
    x = greedy_perm(torch.zeros(B, n1max, n2max, device=scores.device), top, k)
    x = x.to(scores.dtype)
    return (x, out_s.to(scores.dtype)) if return_prob else x


def hungarian(s, n1=None, n2=None, nproc=1):
    """``hungarian(s, n1, n2, nproc)`` (``utils/hungarian.py:8-66``): the optimal assignment
    maximising ``s`` on each pair's valid block (scipy ``linear_sum_assignment`` of ``-s``, same
    tie rules) -> 0/1 matrix of ``s``'s shape, dtype and device.  Solved on the host LSA pool
    (fpm_lsa_batch_host, ``nproc`` threads) as the reference solves it on the host."""
    matrix_input = s.dim() == 2
    if matrix_input:
        s = s.unsqueeze(0)
    elif s.dim() != 3:
        raise ValueError("input data shape not understood: %s" % (tuple(s.shape),))
    B, n1max, n2max = s.shape
    host = s.detach().to("cpu", torch.float32).contiguous()
    a = lsa_batch_host(host, _counts(n1, B, n1max, "cpu"), _counts(n2, B, n2max, "cpu"), max(1, int(nproc)))
    perm = torch.zeros(B, n1max, n2max, dtype=torch.float32)
    r = torch.nonzero(a >= 0)
    perm[r[:, 0], r[:, 1], a[r[:, 0], r[:, 1]].long()] = 1.0
    perm = perm.to(device=s.device, dtype=s.dtype)
    return perm.squeeze(0) if matrix_input else perm


