"""Generate golden vectors from the reference's own importable modules.

Run ONLY in the build container (the reference tree does not exist on the GPU box):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 SPHINX=1 PYTHONPATH=/root/reference:/root/repo \
        python /root/repo/tests/golden/make_golden.py

``SPHINX=1`` is the reference's own switch that skips the nvcc JIT of ``src/extension``
(``src/sparse_torch/csx_matrix.py:7``, ``src/sparse.py:10``).  Only inputs and outputs are
written (``tests/golden/*.npz``); no reference source is copied.  Modules used:
``src.model.soft_topk`` (soft_topk -> Sinkhorn_m, greedy_perm), ``src.model.afau.Encoder``,
``src.model.affinity_layer``, ``src.model.gcn.Gconv``, ``utils.hungarian``,
``utils.build_graphs``, ``utils.factorize_graph_matching`` + ``src.sparse_torch``,
``utils.feature_align``, ``src.loss_func``; and plain-torch pieces of ``src/model/ngm.py`` (which
does not import here) executed from their source text: ``MatchClassifier``, the readout layout and
the forward's tail after the final Sinkhorn; and the stage block of ``train.py`` run against
``fpm.Net`` (``train_stages.json``: parameter names and optimizer settings).  ``python make_golden.py NAME ...`` regenerates only the named fixtures.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

import fpm  # noqa: E402  (seeded params + synthetic graphs; no reference code)
from fpm import params, synth  # noqa: E402

from src.model.soft_topk import soft_topk, greedy_perm  # noqa: E402
from src.model.afau import Encoder  # noqa: E402
from src.model.affinity_layer import InnerProductWithWeightsAffinity  # noqa: E402
from src.model.gcn import Gconv  # noqa: E402
from utils.hungarian import hungarian  # noqa: E402
from utils.build_graphs import build_graphs  # noqa: E402
from utils.factorize_graph_matching import kronecker_sparse, construct_sparse_aff_mat  # noqa: E402
from src.sparse_torch import CSCMatrix3d  # noqa: E402
from utils.feature_align import feature_align  # noqa: E402


def save(name, **arrs):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrs.items()})
    print("wrote", path, sorted(arrs))


def gen_soft_topk():
    g = torch.Generator().manual_seed(11)
    cases = []
    # (n1, n2) per pair; B=3 incl. a ragged pair; scores shaped like Sinkhorn outputs in [0,1]
    for ci, (ns1, ns2) in enumerate([((8, 8, 8), (8, 8, 8)), ((6, 8, 7), (8, 8, 5)), ((16, 12), (16, 14))]):
        B = len(ns1)
        n1m, n2m = max(ns1), max(ns2)
        sc = torch.zeros(B, n1m, n2m)
        for b in range(B):
            sc[b, :ns1[b], :ns2[b]] = torch.rand(ns1[b], ns2[b], generator=g) ** 3
        ks = torch.tensor([min(a, b) * f for a, b, f in list(zip(ns1, ns2, (0.37, 0.62, 0.81)))[:B]],
                          dtype=torch.float32)
        nr, nc = torch.tensor(ns1), torch.tensor(ns2)
        x, ss = soft_topk(sc, ks, 10, 0.01, nr, nc, True)
        cases.append(dict(scores=sc.numpy(), ks=ks.numpy(), n1=nr.numpy(), n2=nc.numpy(),
                          ss_out=ss.numpy(), x=x.numpy()))
    save("soft_topk", **{"c%d_%s" % (i, k): v for i, c in enumerate(cases) for k, v in c.items()},
         ncases=len(cases))


def gen_hungarian_greedy():
    g = torch.Generator().manual_seed(12)
    B, n1, n2 = 3, 9, 10
    s = torch.rand(B, n1, n2, generator=g)
    s[1, :, 7] = 0.0                       # ties
    nr = torch.tensor([9, 7, 9])
    nc = torch.tensor([10, 10, 6])
    x = hungarian(s, nr, nc)
    ks = torch.tensor([4.5, 5.5, 3.2])     # .5 -> half-to-even rounding
    top = torch.argsort(x.mul(s).reshape(B, -1), descending=True, dim=-1)
    perm = greedy_perm(torch.zeros(s.shape), top, ks)
    save("hungarian_greedy", s=s.numpy(), n1=nr.numpy(), n2=nc.numpy(), x=x.numpy(), ks=ks.numpy(),
         top=top.numpy(), perm=perm.numpy())


def gen_encoder():
    sd = params.init_params(5)
    enc = Encoder()
    esd = {k[len("encoder_k."):]: v for k, v in sd.items() if k.startswith("encoder_k.")}
    enc.load_state_dict(esd)
    enc.eval()
    g = torch.Generator().manual_seed(14)
    B, n1m, n2m = 2, 10, 12
    ns2 = [12, 9]
    row = torch.zeros(B, n1m, 600)
    col = torch.zeros(B, n2m, 600)
    for b in range(B):
        col[b, torch.arange(ns2[b]), torch.arange(ns2[b])] = 1
    cost = torch.rand(B, n1m, n2m, generator=g)
    cost[1, :, 9:] = 0
    with torch.no_grad():
        r, c = enc(row, col, cost)
        # general (non-zero) row embedding exercises the q/k path too
        row2 = torch.randn(B, n1m, 600, generator=g) * 0.1
        r2, c2 = enc(row2, col, cost)
    save("afau_encoder", seed=5, row=row.numpy(), col=col.numpy(), cost=cost.numpy(), r=r.numpy(),
         c=c.numpy(), row2=row2.numpy(), r2=r2.numpy(), c2=c2.numpy())


def gen_affinity():
    sd = params.init_params(6)
    aff = InnerProductWithWeightsAffinity(1024, 768)
    aff.A.weight.data.copy_(sd["vertex_affinity.A.weight"])
    aff.A.bias.data.copy_(sd["vertex_affinity.A.bias"])
    g = torch.Generator().manual_seed(15)
    X = [torch.randn(7, 768, generator=g) * 0.05, torch.randn(5, 768, generator=g) * 0.05]
    Y = [torch.randn(9, 768, generator=g) * 0.05, torch.randn(5, 768, generator=g) * 0.05]
    W = torch.rand(2, 1024, generator=g)
    W = W / W.norm(dim=1, keepdim=True)
    with torch.no_grad():
        out = aff(X, Y, W)
    save("affinity", seed=6, X0=X[0].numpy(), X1=X[1].numpy(), Y0=Y[0].numpy(), Y1=Y[1].numpy(),
         W=W.numpy(), K0=out[0].numpy(), K1=out[1].numpy())


def gen_graphs_and_pattern():
    rng = np.random.default_rng(16)
    P1 = np.stack([rng.uniform(0, 320, 9), rng.uniform(0, 240, 9)], 1)
    P2 = np.stack([rng.uniform(0, 320, 7), rng.uniform(0, 240, 7)], 1)
    A1, G1, H1, e1 = build_graphs(P1, 9, stg="tri", sym=True)
    A2, G2, H2, e2 = build_graphs(P2, 7, stg="tri", sym=True)
    # collate (src/gmdataset.py:623-634): per-pair K1G = kron(G2, G1) in CSC, K1H = kron(H2, H1)^T
    n1max = 9
    K1G = [kronecker_sparse(G2, G1).astype(np.float32)]
    K1H = [kronecker_sparse(H2, H1).astype(np.float32)]
    kro_G = CSCMatrix3d(K1G).indices
    kro_H = CSCMatrix3d(K1H).transpose().indices
    Ke = torch.arange(e1 * e2, dtype=torch.float32).view(e1, e2) + 1000
    Kp = torch.arange(9 * 7, dtype=torch.float32).view(9, 7)
    val, row, col = construct_sparse_aff_mat(Ke, Kp, kro_G.float(), kro_H.float())
    save("graphs_pattern", P1=P1, P2=P2, A1=A1, G1=G1, H1=H1, A2=A2, G2=G2, H2=H2, n1max=n1max,
         kro_G=kro_G.numpy(), kro_H=kro_H.numpy(), val=val.numpy(), row=row.numpy(), col=col.numpy())


def gen_pyg_edges():
    """Edge list/pseudo built the way GMDataset.to_pyg_graph does (gmdataset.py:170-189):
    restated in fpm.synth; pin the Delaunay adjacency against build_graphs('tri')."""
    out = {}
    for i, n in enumerate((12, 40)):
        g = synth.make_graph(77, i, 0, n)
        A, G, H, e = build_graphs(g["P"].astype(np.float64), n, stg="tri", sym=True)
        out["c%d_P" % i] = g["P"]
        out["c%d_A" % i] = A
        out["c%d_G" % i] = G
        out["c%d_H" % i] = H
    save("delaunay", ncases=2, **out)


def gen_gconv():
    g = torch.Generator().manual_seed(17)
    torch.manual_seed(17)
    gc = Gconv(6, 5)
    A = (torch.rand(2, 8, 8, generator=g) > 0.6).float()
    x = torch.randn(2, 8, 6, generator=g)
    with torch.no_grad():
        y = gc(A, x)
    save("gconv", A=A.numpy(), x=x.numpy(), a_w=gc.a_fc.weight.detach().numpy(),
         a_b=gc.a_fc.bias.detach().numpy(), u_w=gc.u_fc.weight.detach().numpy(),
         u_b=gc.u_fc.bias.detach().numpy(), y=y.numpy())


def gen_feature_align():
    """utils/feature_align.py on maps of the backbone's spatial sizes (240x320 image: stride-16
    15x20, stride-32 8x10) with keypoints on the borders and outside the frame (clamped /
    nearest-neighbour branches).  Maps are normalised over channels first (ngm.py:65-67)."""
    g = torch.Generator().manual_seed(23)
    nodes = torch.randn(2, 70, 15, 20, generator=g)
    edges = torch.randn(2, 130, 8, 10, generator=g)
    P = torch.rand(2, 9, 2, generator=g) * torch.tensor([320.0, 240.0])
    P[0, 0] = torch.tensor([0.0, 0.0])
    P[0, 1] = torch.tensor([319.9, 239.9])
    P[0, 2] = torch.tensor([-5.0, 250.0])
    P[0, 3] = torch.tensor([10.6, 6.0])
    P[0, 4] = torch.tensor([330.0, -3.0])
    P[1, 0] = torch.tensor([160.0, 120.0])
    ns = torch.tensor([9, 6])
    nn_ = nodes / torch.norm(nodes, dim=1, keepdim=True)
    ne_ = edges / torch.norm(edges, dim=1, keepdim=True)
    U = feature_align(nn_, P, ns, (320, 240))
    F = feature_align(ne_, P, ns, (320, 240))
    save("feature_align", nodes=nodes.numpy(), edges=edges.numpy(), P=P.numpy(), ns=ns.numpy(),
         U=U.numpy(), F=F.numpy())


# ---------------------------------------------------------------------------------------------------
# ngm.py pieces: the module does not import here (torch_geometric / torch_sparse / pygmtools are
# absent), but these blocks are plain torch.  Their source text is executed as written, against
# modules built from the reference's own classes (Encoder) and our seeded parameters; only inputs and
# outputs are stored.
# ---------------------------------------------------------------------------------------------------
NGM = None


def _ngm_lines():
    import inspect
    import src.model.afau as afau_mod
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(inspect.getfile(afau_mod)))))
    path = os.path.join(root, "src", "model", "ngm.py")
    with open(path) as f:
        return path, f.read().split("\n")


def _ngm_class(name):
    """The class ``name`` of ngm.py, compiled from its source lines (ast locates it)."""
    import ast
    import torch.nn as nn
    path, lines = _ngm_lines()
    tree = ast.parse("\n".join(lines))
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name)
    src = "\n".join(lines[node.lineno - 1:node.end_lineno])
    ns = {"torch": torch, "nn": nn}
    exec(compile(src, "%s:%d-%d" % (path, node.lineno, node.end_lineno), "exec"), ns)
    return ns[name], (node.lineno, node.end_lineno)


def _ngm_block(first, last, indent, extra=0):
    """ngm.py lines from the one containing ``first`` through the one containing ``last`` plus
    ``extra`` more (inclusive), dedented by ``indent`` -> (code object, (lineno, end_lineno))."""
    path, lines = _ngm_lines()
    i = next(k for k, l in enumerate(lines) if first in l)
    j = next(k for k in range(i, len(lines)) if last in lines[k]) + extra
    src = "\n".join(l[indent:] if l.startswith(" " * indent) else l.lstrip() for l in lines[i:j + 1])
    return compile(src, "%s:%d-%d" % (path, i + 1, j + 1), "exec"), (i + 1, j + 1)


def _sd_module(mod, sd, prefix):
    mod.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)})
    return mod


def _head_self(sd):
    """An object carrying the attributes the forward tail reads from ``self`` (ngm.py:118-202),
    built from the reference's classes with the seeded parameters ``sd``."""
    import torch.nn as nn
    import types
    MatchClassifier, _ = _ngm_class("MatchClassifier")
    me = types.SimpleNamespace()
    me.univ_size, me.mean_k, me.regression, me.training, me.tau, me.k_factor = 600, True, True, False, 0.01, 50.0
    me.encoder_k = _sd_module(Encoder(), sd, "encoder_k.").eval()
    me.maxpool = nn.MaxPool1d(kernel_size=600)
    for h in ("final_row", "final_col"):
        setattr(me, h, _sd_module(nn.Sequential(nn.Linear(600, 8), nn.ReLU(), nn.Linear(8, 1)), sd, h + "."))
    me.match_cls = _sd_module(MatchClassifier(), sd, "match_cls.").eval()
    me.classifier = _sd_module(nn.Linear(17, 1), sd, "classifier.")
    return me


def gen_match_classifier():
    """MatchClassifier (ngm.py:75-106) from its own source: eval mode with the seeded (non-trivial)
    BatchNorm running statistics, and train mode (batch statistics + the running-buffer update)."""
    sd = params.init_params(8)
    MatchClassifier, span = _ngm_class("MatchClassifier")
    g = torch.Generator().manual_seed(31)
    B, H, W = 3, 12, 14
    m = torch.zeros(B, H, W)
    for b, (h, w) in enumerate(((12, 14), (9, 14), (12, 10))):
        m[b, :h, :w] = torch.randn(h, w, generator=g) * (torch.rand(h, w, generator=g) < 0.3)
    mc = _sd_module(MatchClassifier(), sd, "match_cls.")
    with torch.no_grad():
        mc.eval()
        logits_eval = mc(m)
        mc.train()
        logits_train = mc(m)
    run = {k: v.detach().numpy() for k, v in mc.state_dict().items() if "running" in k}
    save("match_classifier", seed=8, span=np.array(span), m=m.numpy(), logits_eval=logits_eval.numpy(),
         logits_train=logits_train.numpy(), **{"after_" + k.replace(".", "_"): v for k, v in run.items()})


def _tail_inputs(seed, n1, n2):
    """Readout scores s and their Sinkhorn ss for a ragged batch (inputs only: any valid ss works)."""
    import oracle as O
    g = torch.Generator().manual_seed(seed)
    B = len(n1)
    n1m, n2m = max(n1), max(n2)
    s = torch.zeros(B, n1m, n2m)
    for b in range(B):
        s[b, :n1[b], :n2[b]] = torch.randn(n1[b], n2[b], generator=g) * 0.02
        k = min(n1[b], n2[b])
        s[b, torch.arange(k), torch.randperm(n2[b], generator=g)[:k]] += 0.03
    ss = O.pygm_sinkhorn(s, n1, n2, dummy_row=True, max_iter=10, tau=0.01)
    return s, ss


def gen_ngm_tail():
    """The forward after the final Sinkhorn (ngm.py: from the min_point_list line through the
    data_dict.update): AFA-U k head (Encoder + -inf pad + MaxPool1d + final_row/col + mean +
    sigmoid), soft_topk with the predicted k, hungarian, argsort + greedy_perm, MatchClassifier on
    s * perm, and the losses -- executed from the reference's source with ss, s as inputs.  Also the
    readout layout v = classifier(emb); s = v.view(B, n2max, -1).transpose(1, 2) (ngm.py:368-369)."""
    sd = params.init_params(8)
    me = _head_self(sd)
    out = {"seed": 8}
    cases = [((10, 8, 12), (12, 12, 9), 41), ((16, 16), (16, 16), 42), ((7, 13, 11, 13), (13, 9, 13, 12), 43)]
    code, span = _ngm_block("# Calculate the minimum number of keypoints", "'k_prob': ks,", 8, extra=1)
    out["span"] = np.array(span)
    for ci, (n1, n2, seed) in enumerate(cases):
        B = len(n1)
        s, ss = _tail_inputs(seed, list(n1), list(n2))
        gt = torch.zeros(B, max(n1), max(n2))
        for b in range(B):
            k = min(n1[b], n2[b]) - (b % 3)
            gt[b, torch.arange(k), torch.arange(k)] = 1.0
        label = torch.tensor([float(b % 2) for b in range(B)])
        dd = {"gt_perm_mat": gt, "label": label}
        ns = {"self": me, "torch": torch, "s": s, "ss": ss, "data_dict": dd, "batch_size": B, "idx1": 0, "idx2": 1,
              "n_points": [torch.tensor(n1), torch.tensor(n2)], "SK_ITER_NUM": 10, "soft_topk": soft_topk,
              "hungarian": hungarian, "greedy_perm": greedy_perm, "s_list": [], "x_list": [], "indices": []}
        with torch.no_grad():
            exec(code, ns)
        # the reference orders matches by torch's unstable argsort; keep cases where the stable order
        # (the oracle's) selects the same matches, so the fixture pins one well-defined answer
        x_l = hungarian(ns["ss_out"], torch.tensor(n1), torch.tensor(n2))
        top_s = torch.argsort(x_l.mul(ns["ss_out"]).reshape(B, -1), descending=True, dim=-1, stable=True)
        perm_s = greedy_perm(torch.zeros(ns["ss_out"].shape), top_s, ns["ks"].view(-1) * ns["min_point_tensor"])
        assert torch.equal(perm_s, dd["perm_mat"]), "case %d: argsort tie at the greedy cut" % ci
        for k, v in (("n1", torch.tensor(n1)), ("n2", torch.tensor(n2)), ("s", s), ("ss", ss), ("gt", gt),
                     ("label", label), ("ks", dd["k_prob"]), ("ds_mat", dd["ds_mat"]), ("perm", dd["perm_mat"]),
                     ("cls_logits", ns["cls_logits"]), ("cls_prob", dd["cls_prob"]), ("ks_loss", dd["ks_loss"]),
                     ("ks_error", dd["ks_error"]), ("cls_loss", dd["cls_loss"])):
            out["c%d_%s" % (ci, k)] = torch.as_tensor(v).detach().numpy()
    out["ncases"] = len(cases)
    # readout layout (ngm.py:368-369)
    rcode, rspan = _ngm_block("v = self.classifier(emb)", "s = v.view(v.shape[0]", 8)
    g = torch.Generator().manual_seed(44)
    B, n1m, n2m = 2, 5, 7
    emb = torch.randn(B, n1m * n2m, 17, generator=g)
    rns = {"self": me, "emb": emb, "points": [torch.zeros(B, n1m, 2), torch.zeros(B, n2m, 2)], "idx2": 1}
    with torch.no_grad():
        exec(rcode, rns)
    out.update(readout_span=np.array(rspan), readout_emb=emb.numpy(), readout_n1max=n1m, readout_n2max=n2m,
               readout_s=rns["s"].numpy())
    save("ngm_tail", **out)


def gen_permutation_loss():
    """PermutationLoss (src/loss_func.py:26-59) on a ragged batch."""
    from src.loss_func import PermutationLoss
    g = torch.Generator().manual_seed(45)
    n1, n2 = torch.tensor([6, 4, 5]), torch.tensor([6, 6, 3])
    ds = torch.rand(3, 6, 6, generator=g) * 0.98 + 0.01
    gt = torch.zeros(3, 6, 6)
    for b in range(3):
        k = int(min(n1[b], n2[b]))
        gt[b, torch.arange(k), torch.randperm(k, generator=g)] = 1.0
    loss = PermutationLoss()(ds, gt, n1, n2)
    save("permutation_loss", ds=ds.numpy(), gt=gt.numpy(), n1=n1.numpy(), n2=n2.numpy(), loss=loss.numpy())


def gen_train_stages():
    """train.py:153-239 (the stage block: freeze / unfreeze per stage and the optimizers it builds),
    executed unchanged from the reference's source text against ``fpm.Net`` for stages 1-6.  Stored
    (train_stages.json): per stage the names of the parameters left trainable and, per optimizer, each
    group's parameter names, lr and weight decay -- names and numbers only."""
    import json
    import torch.optim as optim
    path = os.path.join(os.path.dirname(_ngm_lines()[0]), "..", "..", "train.py")
    with open(path) as f:
        lines = f.read().split("\n")
    block = lines[152:239]
    assert "backbone_ids" in block[4] and "optimizer_cls" in block[-1], "train.py moved"
    code = compile("\n".join(l[4:] if l.startswith("    ") else l for l in block), path + ":153-239", "exec")
    hyper = {"LR": 1e-3, "BACKBONE_LR": 1e-5, "K_LR": 1e-4}
    out = {"hyper": hyper, "stages": {}}
    for stage in range(1, 7):
        model = fpm.Net(regression=True)
        names = {id(p): n for n, p in model.named_parameters()}
        ns = dict(hyper, model=model, stage=stage, optim=optim, torch=torch, print=lambda *a, **k: None)
        exec(code, ns)

        def groups(opt):
            return None if opt is None else [{"params": sorted(names[id(p)] for p in g["params"]), "lr": g["lr"],
                                              "weight_decay": g["weight_decay"]} for g in opt.param_groups]
        out["stages"][str(stage)] = {"trainable": sorted(n for n, p in model.named_parameters() if p.requires_grad),
                                     "optimizer": groups(ns["optimizer"]), "optimizer_k": groups(ns["optimizer_k"])}
    with open(os.path.join(HERE, "train_stages.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("wrote train_stages.json")


GENERATORS = dict(soft_topk=gen_soft_topk, hungarian_greedy=gen_hungarian_greedy, encoder=gen_encoder,
                  affinity=gen_affinity, graphs_pattern=gen_graphs_and_pattern, delaunay=gen_pyg_edges,
                  gconv=gen_gconv, feature_align=gen_feature_align, match_classifier=gen_match_classifier,
                  ngm_tail=gen_ngm_tail, permutation_loss=gen_permutation_loss, train_stages=gen_train_stages)

if __name__ == "__main__":
    for name in (sys.argv[1:] or list(GENERATORS)):
        GENERATORS[name]()
