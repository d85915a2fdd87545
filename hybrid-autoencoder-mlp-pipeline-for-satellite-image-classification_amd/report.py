"""Reporting helpers of the reference workflow: the validation-loss heat-map table of the alpha x lr grid
(R.md:2415-2425), the loss curves (R.md:2460-2469), the confusion matrix (R.md:3188-3190) and the per-class report the
notebook prints with sklearn's `classification_report(..., digits=4)` (R.md:3216-3237).

Numbers only, computed with NumPy (sklearn is not needed to get them).  Drawing the figures is out of scope (SURVEY.md section 2:
plotting).
"""
import json

import numpy as np


def load_validation_losses(path="models_best/validation_losses.json"):
    """The JSON written by `grid_search_autoencoder` / the reference (R.md:718-729): {"alpha=A, lr=LR": best_val_loss}."""
    with open(path, "r") as f:
        return json.load(f)


def loss_heatmap(results, alpha_values, lr_values):
    """heatmap[i, j] = best validation loss of (alpha_values[i], lr_values[j])   (R.md:2419-2425)."""
    hm = np.zeros((len(alpha_values), len(lr_values)))
    for i, a in enumerate(alpha_values):
        for j, lr in enumerate(lr_values):
            hm[i, j] = results[f"alpha={a}, lr={lr}"]
    return hm


def best_config(results):
    """(alpha, lr, loss) of the lowest validation loss; first entry wins ties, as in the reference's strict `<` (R.md:701)."""
    best = None
    for key, v in results.items():
        if best is None or v < best[2]:
            a, lr = key.split(", ")
            best = (float(a.split("=")[1]), float(lr.split("=")[1]), v)
    return best


def confusion_matrix(labels, preds, num_classes=None):
    """cm[i, j] = number of samples of true class i predicted as j (sklearn.metrics.confusion_matrix semantics for integer
    classes; when num_classes is None the classes are the sorted union of labels and predictions)."""
    labels = np.asarray(labels).astype(np.int64).ravel()
    preds = np.asarray(preds).astype(np.int64).ravel()
    if labels.shape != preds.shape:
        raise ValueError("labels and preds must have the same length")
    if num_classes is None:
        classes = np.unique(np.concatenate([labels, preds]))
        idx = {c: i for i, c in enumerate(classes.tolist())}
        li = np.array([idx[c] for c in labels.tolist()], dtype=np.int64)
        pi = np.array([idx[c] for c in preds.tolist()], dtype=np.int64)
        n = len(classes)
    else:
        li, pi, n = labels, preds, int(num_classes)
    cm = np.zeros((n, n), dtype=np.int64)
    np.add.at(cm, (li, pi), 1)
    return cm


def class_metrics(labels, preds):
    """Per-class precision / recall / f1 / support plus accuracy, macro and weighted averages (zero_division -> 0)."""
    labels = np.asarray(labels).astype(np.int64).ravel()
    preds = np.asarray(preds).astype(np.int64).ravel()
    classes = np.unique(np.concatenate([labels, preds]))
    cm = confusion_matrix(labels, preds)
    tp = np.diag(cm).astype(np.float64)
    pred_n = cm.sum(0).astype(np.float64)
    true_n = cm.sum(1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        prec = np.where(pred_n > 0, tp / pred_n, 0.0)
        rec = np.where(true_n > 0, tp / true_n, 0.0)
        f1 = np.where(prec + rec > 0, 2 * prec * rec / (prec + rec), 0.0)
    total = true_n.sum()
    w = true_n / max(total, 1.0)
    return {
        "classes": classes, "precision": prec, "recall": rec, "f1": f1, "support": true_n.astype(np.int64),
        "accuracy": float(tp.sum() / max(total, 1.0)),
        "macro": (float(prec.mean()), float(rec.mean()), float(f1.mean())),
        "weighted": (float((prec * w).sum()), float((rec * w).sum()), float((f1 * w).sum())),
        "total": int(total),
    }


def confusion_metrics(cm, num_classes=None):
    """Per-class and overall accuracy figures of a confusion matrix of pixel (or sample) counts, NumPy array or tensor: the [K+1,K+1]
    matrix of `scene.scene_confusion` (row K: unlabelled truth, column K: not classified; num_classes=None takes K = n - 1), or a
    plain [K,K] one (``num_classes=K``).  With M = cm[:K,:K], u = cm[:K,K] and a = cm[K,:K]:

    support_c = sum M[c,:] + u_c (a labelled pixel the map left unclassified is an omission); recall (producer's accuracy) =
    M[c,c] / support_c; precision (user's accuracy) = M[c,c] / sum M[:,c]; f1; iou = M[c,c] / (support_c + sum M[:,c] - M[c,c]);
    accuracy = trace / sum support; kappa = Cohen's over the labelled rows, "not classified" being a predicted category without a
    true row; macro / weighted averages as `class_metrics`; unclassified = u; area = cm[:, :K].sum(0), the pixels mapped to each
    class, unlabelled truth included.  Zero division gives 0."""
    if hasattr(cm, "detach"):
        cm = cm.detach().cpu().numpy()
    cm = np.asarray(cm)
    if cm.ndim != 2 or cm.shape[0] != cm.shape[1] or cm.shape[0] < 1:
        raise ValueError("cm must be a square matrix")
    n = cm.shape[0]
    k = n - 1 if num_classes is None else int(num_classes)
    if k < 1 or n not in (k, k + 1):
        raise ValueError(f"cm must be [K,K] or [K+1,K+1] with K = {k}, got {list(cm.shape)}")
    cm = cm.astype(np.int64)
    m = cm[:k, :k]
    u = cm[:k, k] if n > k else np.zeros(k, dtype=np.int64)
    tp = np.diag(m).astype(np.float64)
    pred_n = m.sum(0).astype(np.float64)
    true_n = (m.sum(1) + u).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        prec = np.where(pred_n > 0, tp / pred_n, 0.0)
        rec = np.where(true_n > 0, tp / true_n, 0.0)
        f1 = np.where(prec + rec > 0, 2 * prec * rec / (prec + rec), 0.0)
        union = true_n + pred_n - tp
        iou = np.where(union > 0, tp / union, 0.0)
    total = true_n.sum()
    w = true_n / max(total, 1.0)
    po = tp.sum() / max(total, 1.0)
    pe = float((true_n * pred_n).sum()) / max(total * total, 1.0)          # column K has no true row: its product is 0
    return {
        "classes": np.arange(k), "precision": prec, "recall": rec, "f1": f1, "iou": iou, "support": true_n.astype(np.int64),
        "accuracy": float(po), "kappa": float((po - pe) / (1.0 - pe)) if pe < 1.0 else 0.0,
        "macro": (float(prec.mean()), float(rec.mean()), float(f1.mean())),
        "weighted": (float((prec * w).sum()), float((rec * w).sum()), float((f1 * w).sum())),
        "mean_iou": float(iou.mean()), "unclassified": u.copy(), "area": cm[:, :k].sum(0), "total": int(total),
    }


def cluster_class_table(cluster_labels, class_labels, k, num_classes):
    """Contingency counts of clusters against classes: int64 [k, num_classes], entry (q, c) = the number of positions with cluster q
    and class c.  Both arguments are integer tensors of one shape (CPU or GPU: plain torch), e.g. the cluster map of
    `cluster.cluster_scene` and the labels of `scene.window_labels`; a pair with either label outside its range (-1: window not run,
    unlabelled) is skipped."""
    import torch
    if cluster_labels.shape != class_labels.shape:
        raise ValueError("cluster_labels and class_labels must have the same shape")
    k, num_classes = int(k), int(num_classes)
    if k < 1 or num_classes < 1:
        raise ValueError("k and num_classes must be positive")
    q = cluster_labels.reshape(-1).to(torch.int64)
    c = class_labels.reshape(-1).to(torch.int64).to(q.device)
    ok = (q >= 0) & (q < k) & (c >= 0) & (c < num_classes)
    # a skipped pair goes to the extra bin k * num_classes, dropped below (no boolean indexing: nothing is read back on a GPU)
    flat = torch.where(ok, q * num_classes + c, k * num_classes)
    return torch.zeros(k * num_classes + 1, dtype=torch.int64, device=q.device).scatter_add_(0, flat, torch.ones_like(flat))[:-1].reshape(
        k, num_classes)


def name_clusters(table):
    """The majority class of every cluster of a `cluster_class_table`: int64 [k], the lowest class on a tie, -1 for a cluster whose row
    is empty."""
    import torch
    best = torch.argmax((table == table.max(dim=1, keepdim=True).values).to(torch.int64), dim=1)      # the first maximum
    return torch.where(table.sum(dim=1) > 0, best, -1)


def separation_table(matrix, per_class, names=None, digits=4):
    """Text table of how the classes sit in the latent space, one line per class: its silhouette (`validity.silhouette_score`'s
    per_class), its mean intra-class distance (the diagonal of `validity.class_distance_matrix`), the nearest other class by mean
    distance, that distance, and the ratio inter / intra (above 1: the class is closer to itself than to its nearest neighbour).
    matrix [K, K] and per_class [K] are NumPy arrays or tensors; names: K strings (default: the class ids).  A class whose row is NaN
    (empty) has '-' in every column, as has a figure that does not exist (a class of one row has no intra-class distance)."""
    if hasattr(matrix, "detach"):
        matrix = matrix.detach().cpu().numpy()
    if hasattr(per_class, "detach"):
        per_class = per_class.detach().cpu().numpy()
    matrix = np.asarray(matrix, dtype=np.float64)
    per_class = np.asarray(per_class, dtype=np.float64).ravel()
    if matrix.ndim != 2 or matrix.shape[0] != matrix.shape[1] or matrix.shape[0] < 1:
        raise ValueError("matrix must be a square [K, K] matrix")
    k = matrix.shape[0]
    if per_class.shape[0] != k:
        raise ValueError(f"per_class must have {k} entries, got {per_class.shape[0]}")
    names = [str(c) for c in range(k)] if names is None else [str(n) for n in names]
    if len(names) != k:
        raise ValueError(f"names must have {k} entries, got {len(names)}")
    width = max(max(len(n) for n in names), len("class"))

    def num(v):
        return "{:>10}".format("-") if not np.isfinite(v) else "{:>10.{d}f}".format(v, d=digits)

    head = "{:>{w}s} ".format("class", w=width) + " {:>10} {:>10} {:>{w}s} {:>10} {:>10}".format("silhouette", "intra", "nearest", "inter", "ratio",
                                                                                              w=width)
    lines = [head, ""]
    for a in range(k):
        inter = matrix[a].copy()
        inter[a] = np.nan
        if np.isfinite(inter).any():
            b = int(np.nanargmin(inter))                       # the first minimum: the lowest class id on a tie
            near, dist = names[b], inter[b]
        else:
            near, dist = "-", np.nan
        intra = matrix[a, a]
        ratio = dist / intra if np.isfinite(dist) and np.isfinite(intra) and intra > 0 else np.nan
        lines.append("{:>{w}s} ".format(names[a], w=width) + " " + num(per_class[a]) + " " + num(intra) + " {:>{w}s}".format(near, w=width)
                     + " " + num(dist) + " " + num(ratio))
    return "\n".join(lines) + "\n"


def zone_table(stats, labels, class_names=None, digits=4):
    """Text table of an object-based classification, one line per zone: its id, its pixels (votes.sum(1)), the share of them that
    was classified, its class and the confidence.  stats: `zonal.ZonalStats` (only votes is read); labels: what `zonal.zone_labels`
    returned, (label, confidence, coverage); class_names: K strings (default: the class ids).  A zone without a label, and a figure
    that does not exist (NaN), print as '-'."""
    def host(t):
        return np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t)

    votes = host(stats.votes)
    if votes.ndim != 2 or votes.shape[1] < 2:
        raise ValueError("stats.votes must be a [Z, K+1] table")
    z, k = votes.shape[0], votes.shape[1] - 1
    try:
        label, confidence, coverage = (host(t).ravel() for t in labels)
    except (TypeError, ValueError):
        raise ValueError("labels must be the (label, confidence, coverage) triple of zone_labels") from None
    if not (label.shape[0] == confidence.shape[0] == coverage.shape[0] == z):
        raise ValueError(f"labels must have {z} entries each, one per zone")
    names = [str(c) for c in range(k)] if class_names is None else [str(n) for n in class_names]
    if len(names) != k:
        raise ValueError(f"class_names must have {k} entries, got {len(names)}")
    width = max(max(len(n) for n in names), len("class"))

    def num(v):
        return "{:>10}".format("-") if not np.isfinite(v) else "{:>10.{d}f}".format(v, d=digits)

    lines = ["{:>8} {:>10} {:>10} {:>{w}s} {:>10}".format("zone", "pixels", "coverage", "class", "confidence", w=width), ""]
    pixels = votes.sum(1)
    for i in range(z):
        c = int(label[i])
        lines.append("{:>8} {:>10} ".format(i, int(pixels[i])) + num(coverage[i]) + " {:>{w}s} ".format(names[c] if 0 <= c < k else "-", w=width)
                     + num(confidence[i]))
    return "\n".join(lines) + "\n"


def transition_table(table, class_names=None):
    """Text table of a post-classification comparison, one line per class: its pixels at date A and at date B, how many kept the
    class, and the class that took the most of what it lost and the one that gave the most of what it gained (with the counts).
    table: `change.class_transitions`' [K+1, K+1] counts, rows = date A, columns = date B, index K = no class ("-" in the table);
    class_names: K strings (default: the class ids).  A class that lost or gained nothing prints '-'."""
    t = np.asarray(table.detach().cpu().numpy() if hasattr(table, "detach") else table)
    if t.ndim != 2 or t.shape[0] != t.shape[1] or t.shape[0] < 2:
        raise ValueError("table must be a [K+1, K+1] from-to table")
    k = t.shape[0] - 1
    names = [str(c) for c in range(k)] if class_names is None else [str(n) for n in class_names]
    if len(names) != k:
        raise ValueError(f"class_names must have {k} entries, got {len(names)}")
    names = names + ["-"]
    width = max(max(len(n) for n in names), len("class"))

    def top(v, own):
        v = v.copy()
        v[own] = 0
        j = int(v.argmax())                                  # the lowest index on a tie
        return "{:>{w}s} {:>10}".format(names[j], int(v[j]), w=width) if v[j] > 0 else "{:>{w}s} {:>10}".format("-", "-", w=width)

    lines = ["{:>{w}s} {:>10} {:>10} {:>10} {:>{v}s} {:>{v}s}".format("class", "date A", "date B", "kept", "lost to", "gained from",
                                                                      w=width, v=width + 11), ""]
    for c in range(k):
        lines.append("{:>{w}s} {:>10} {:>10} {:>10} ".format(names[c], int(t[c].sum()), int(t[:, c].sum()), int(t[c, c]), w=width)
                     + top(t[c], c) + " " + top(t[:, c], c))
    return "\n".join(lines) + "\n"


def registration_table(registration, shape=None):
    """Text summary of a `register.Registration`: the matrix (a point (x, y) of scene A -> its place in scene B), the shift it gives
    at the scene centre (shape = (H, W); default: at the origin), the rmse of the inliers and how many tiles they are."""
    m = np.asarray(registration.matrix, dtype=np.float64)
    if m.shape != (2, 3):
        raise ValueError("registration.matrix must be 2 x 3")
    x, y = (0.0, 0.0) if shape is None else ((shape[1] - 1) / 2.0, (shape[0] - 1) / 2.0)
    dx, dy = m[0, 0] * x + m[0, 1] * y + m[0, 2] - x, m[1, 0] * x + m[1, 1] * y + m[1, 2] - y
    lines = ["{:>12s} {:>14s} {:>14s} {:>14s}".format("", "x", "y", "1"), ""]
    for name, row in zip(("x in B", "y in B"), m):
        lines.append("{:>12s} {:>14.8f} {:>14.8f} {:>14.5f}".format(name, *row))
    lines += ["", "{:>12s} {}".format("model", registration.model),
              "{:>12s} dx {:+.4f}  dy {:+.4f} px at {}".format("shift", dx, dy, "the origin" if shape is None else "the scene centre"),
              "{:>12s} {:.4f} px".format("rmse", float(registration.rmse)),
              "{:>12s} {} of {} tiles".format("inliers", int(np.asarray(registration.inliers).sum()), int(registration.n_tiles))]
    return "\n".join(lines) + "\n"


def classification_report_from_confusion(cm, digits=4, num_classes=None):
    """`classification_report`'s table from a confusion matrix (`confusion_metrics`: the same matrix forms)."""
    return _report_text(confusion_metrics(cm, num_classes), digits)


def classification_report(labels, preds, digits=4):
    """Text table in the layout sklearn prints for the notebook's call (R.md:3216-3237)."""
    return _report_text(class_metrics(labels, preds), digits)


def _report_text(m, digits):
    names = [str(c) for c in m["classes"].tolist()]
    width = max(max(len(n) for n in names), len("weighted avg"), digits)
    head = "{:>{w}s} ".format("", w=width) + "".join(" {:>9}".format(h) for h in ("precision", "recall", "f1-score", "support"))
    lines = [head, ""]
    row = "{:>{w}s} " + " {:>9.{d}f}" * 3 + " {:>9}"
    for i, n in enumerate(names):
        lines.append(row.format(n, m["precision"][i], m["recall"][i], m["f1"][i], int(m["support"][i]), w=width, d=digits))
    lines.append("")
    lines.append("{:>{w}s} ".format("accuracy", w=width) + " {:>9} {:>9}".format("", "") + " {:>9.{d}f} {:>9}".format(m["accuracy"], m["total"], d=digits))
    lines.append(row.format("macro avg", *m["macro"], m["total"], w=width, d=digits))
    lines.append(row.format("weighted avg", *m["weighted"], m["total"], w=width, d=digits))
    return "\n".join(lines) + "\n"
