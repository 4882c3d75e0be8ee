"""Records ``verification_metrics.npz`` once: 300 scores with ties, their labels, and scikit-learn's outputs for
the reference's evaluation (evaluate_binary_classifier.py:141-159).  Needs scikit-learn (recorded with 1.7); the
test that reads the file does not.

    python tests/golden/make_metrics_golden.py
"""
import os

import numpy as np
from sklearn.metrics import (accuracy_score, auc, confusion_matrix, f1_score, precision_recall_curve, precision_score,
                             recall_score, roc_curve)

rng = np.random.default_rng(20240607)
label = (rng.random(300) < 0.35).astype(np.int64)
# overlapping classes, rounded to two decimals: many ties, inside a class and across the two
prob = np.clip(np.round(rng.normal(0.35 + 0.3 * label, 0.18), 2), 0.0, 1.0)

fpr, tpr, thresholds = roc_curve(label, prob)
fnr = 1 - tpr
eer_idx = np.nanargmin(np.abs(fnr - fpr))
eer_threshold = thresholds[eer_idx]
preds = (prob >= eer_threshold).astype(np.int32)
prec_curve, rec_curve, _ = precision_recall_curve(label, prob)
tn, fp, fn, tp = confusion_matrix(label, preds).ravel()
out = dict(prob=prob, label=label, fpr=fpr, tpr=tpr, thresholds=thresholds, eer_threshold=eer_threshold,
           counts=np.array([tn, fp, fn, tp], dtype=np.int64),
           accuracy=accuracy_score(label, preds), precision=precision_score(label, preds),
           recall=recall_score(label, preds), f1=f1_score(label, preds), roc_auc=auc(fpr, tpr),
           pr_auc=auc(rec_curve, prec_curve), far=fp / (fp + tn), frr=fn / (tp + fn))
np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "verification_metrics.npz"), **out)
print({k: (v if np.ndim(v) == 0 else np.shape(v)) for k, v in out.items()})
