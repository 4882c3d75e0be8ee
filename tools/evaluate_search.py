"""The stage funnel of the 1:N search on a labelled synthetic gallery.

    python tools/evaluate_search.py [--subjects 256] [--mated 32] [--non-mated 8] [--layout f32]
                                    [--shortlist 16] [--prescreen 64] [--by subject] [--far 1e-2]

The gallery holds one ``synth`` graph per subject; the mated probes are second impressions of the first ``--mated``
subjects (a few keypoints dropped, the rest jittered, features perturbed, the graph rebuilt), the non-mated probes
are graphs of subjects that were never enrolled.  Prints ``stage_ranks`` (the mate's rank at the descriptor, coarse
and subject stages), ``search_report`` (which stage of the query lost each mate) and a ``score_report`` of the
coarse scores.

The weights are ``init_params`` (random) with a spread affinity bias: the figures exercise the instrument and say
nothing about accuracy.  Load a trained checkpoint (``--weights``) for numbers that mean something.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import fpm  # noqa: E402
from fpm import evaluate, params, synth  # noqa: E402


def second_impression(g, seed, drop=3, jitter=1.0, noise=0.01):
    """Another impression of graph ``g``: ``drop`` keypoints missing, the rest moved by N(0, jitter px), features
    plus N(0, noise), Delaunay rebuilt, the same global feature."""
    rng = np.random.default_rng(seed)
    keep = np.sort(rng.permutation(g["n"])[:g["n"] - drop])
    P = (g["P"][keep].astype(np.float64) + rng.normal(0, jitter, (keep.size, 2))).astype(np.float32).astype(np.float64)
    A = synth.delaunay_adjacency(P)
    ei, pseudo = synth.edges_from_adjacency(A, P)
    x = (g["x"][keep] + rng.normal(0, noise, g["x"][keep].shape)).astype(np.float32)
    return dict(P=P.astype(np.float32), A=A.astype(np.float32), edge_index=ei, pseudo=pseudo, x=x, w=g["w"].copy(),
                n=int(keep.size))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--subjects", type=int, default=256)
    ap.add_argument("--mated", type=int, default=32)
    ap.add_argument("--non-mated", type=int, default=8)
    ap.add_argument("--layout", default="f32")
    ap.add_argument("--shortlist", type=int, default=16)
    ap.add_argument("--prescreen", type=int, default=64)
    ap.add_argument("--by", default=None, choices=[None, "subject"])
    ap.add_argument("--far", type=float, default=1e-2)
    ap.add_argument("--weights", default=None, help="a state dict saved with torch.save (default: init_params)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.weights:
        sd = torch.load(a.weights, map_location="cpu", weights_only=True)
    else:
        sd = params.init_params(7)
        sd["vertex_affinity.A.bias"] = torch.full_like(sd["vertex_affinity.A.bias"], 2.0)
        print("NOTE: random init_params weights -- the figures below exercise the instrument and mean nothing about "
              "accuracy; pass --weights for a trained checkpoint")
    net = fpm.Net(regression=True, backbone=False)
    net.load_state_dict(sd)
    ns = np.random.default_rng(0).integers(24, 49, size=a.subjects + a.non_mated)
    graphs = [synth.make_graph(42, p, 1, int(n)) for p, n in enumerate(ns)]
    probes = [second_impression(graphs[p], 1000 + p) for p in range(a.mated)] + graphs[a.subjects:]
    index = net.enroll(graphs[:a.subjects], dev, layout=a.layout, descriptors=True, subjects=list(range(a.subjects)))
    pset = net.enroll(probes, dev, descriptors=True,
                      subjects=list(range(a.mated)) + list(range(a.subjects, a.subjects + a.non_mated)))
    print("gallery: %d entries (%s), probes: %d mated, %d non-mated" % (index.G, a.layout, a.mated, a.non_mated))

    sr = net.stage_ranks(pset, index)
    for stage in sr["stages"]:
        print("stage %-15s recall@1 %.3f  @%d %.3f  @%d %.3f   worst rank %d" % (
            stage, sr.recall(stage, 1), a.shortlist, sr.recall(stage, a.shortlist), a.prescreen,
            sr.recall(stage, a.prescreen), int(sr[stage]["mate_rank"].max())))

    query = dict(shortlist=a.shortlist, by=a.by)
    if a.by is None:
        query["prescreen"] = a.prescreen
    rep = net.evaluate_search(pset, index, ks=(1, 5, 10), **query)
    print("query %s: survival %s  cmc %s" % (query, rep["stages"], rep["cmc"]))

    coarse = net.coarse_scores_many(pset, index)
    labels, col = torch.unique(index.subject, return_inverse=True)
    place = {int(v): i for i, v in enumerate(labels.tolist())}
    row = torch.tensor([place.get(int(v), -1) for v in pset.subject.tolist()], dtype=torch.int32, device=dev)
    rs = evaluate.score_report(coarse, row, col.to(torch.int32).to(dev), far=(a.far,))
    t = rs["thresholds"][0]
    print("coarse scores: %d genuine, %d impostor; EER %s; FAR %.3g -> threshold %.6g (achieved FAR %.3g, FRR %.3g)" % (
        t["genuines"], t["impostors"], rs["eer"], a.far, t["threshold"], t["far"], t["frr"]))
    # with the threshold (raw exact scores are another scale: this is the coarse score's) the decision rates
    rep = net.evaluate_search(pset, index, threshold=0.5, **query)
    print("exact stage at threshold 0.5: FNIR %.3f  FPIR %.3f" % (rep["fnir"], rep["fpir"]))
