"""fp64 Lloyd step on the CPU: the reference of csrc/vq.hip (gsr_vq_assign, gsr_vq_update) and of gsr_scene.compress, with the bars and the case
generators that tests/test_vq_cpu.py (host build) and tests/test_gpu_vq.py (device) share.  Test infrastructure.

Bars (none comes from what the kernels give):
  assignment  d64(x, c_got) <= d64(x, c_best) + gamma (|x|^2 + |c_got|^2 + |c_best|^2),  gamma = (D + 4) 2^-23: the kernel compares fp32 scores
              |c|^2 - 2 x.c, each two dot-product chains of length <= D + 1 (error <= (D + 1) u (|x|^2 + |c|^2) per score with u = 2^-24, by
              2 |x.c| <= |x|^2 + |c|^2 term by term) and a choice between two scores can be wrong by the sum of their errors.
  dist2       |dist2 - d64(x, c_got)| <= (D + 4) 2^-24 d64: D subtractions, D fused multiply-adds on non-negative terms.
  update      1 ulp of fp32 at the fp64 weighted mean / mass (the kernel sums in fp64 and rounds once: half an ulp plus the fp64 noise)."""
import numpy as np
import torch

KINDS = {"centred": 0.0, "offset10": 10.0, "offset1000": 1000.0}


def gamma(D):
    return (D + 4) * 2.0 ** -23


def dist2_bar(D):
    return (D + 4) * 2.0 ** -24


def ulp32(v):
    """The spacing of fp32 at |v| (fp64 array in, fp64 out; the smallest normal's spacing below it)."""
    a = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 23)


def pairwise64(rows, codebook):
    """[P,K] squared distances in fp64 from the differences themselves (no score form)."""
    x, c = np.asarray(rows, dtype=np.float64), np.asarray(codebook, dtype=np.float64)
    out = np.empty((x.shape[0], c.shape[0]))
    step = max(1, (1 << 22) // max(1, c.shape[0] * x.shape[1]))
    for i in range(0, x.shape[0], step):
        d = x[i:i + step, None, :] - c[None, :, :]
        out[i:i + step] = (d * d).sum(axis=2)
    return out


def assign64(rows, codebook):
    """-> idx [P] int32 (the LOWEST index among equal distances; -1 for a row with a non-finite component, and for every row when no centroid is
    finite), dist2 [P] fp64 (0 where idx is -1).  A centroid with a non-finite component is never chosen."""
    x, c = np.asarray(rows, dtype=np.float64), np.asarray(codebook, dtype=np.float64)
    row_ok, cen_ok = np.isfinite(x).all(axis=1), np.isfinite(c).all(axis=1)
    d = pairwise64(np.where(row_ok[:, None], x, 0.0), np.where(cen_ok[:, None], c, 0.0))
    d[:, ~cen_ok] = np.inf
    idx = d.argmin(axis=1).astype(np.int32)      # (numpy: the first of equal minima)
    best = d[np.arange(x.shape[0]), idx]
    lost = ~row_ok | ~np.isfinite(best)
    idx[lost] = -1
    return idx, np.where(lost, 0.0, best)


def clean_weights(weights, P):
    if weights is None:
        return np.ones(P)
    w = np.asarray(weights, dtype=np.float64)
    return np.where(np.isfinite(w) & (w > 0), w, 0.0)


def update64(rows, weights, idx, codebook):
    """-> (codebook' [K,D] fp64, mass [K] fp64): weighted means of the rows of every cluster; idx outside [0, K) belongs to nobody; a cluster
    without weight keeps its centroid and has mass 0."""
    x, c = np.asarray(rows, dtype=np.float64), np.array(codebook, dtype=np.float64)
    K = c.shape[0]
    w = clean_weights(weights, x.shape[0])
    idx = np.asarray(idx)
    use = (idx >= 0) & (idx < K) & (w > 0)
    mass = np.bincount(idx[use], weights=w[use], minlength=K)
    sums = np.zeros_like(c)
    np.add.at(sums, idx[use], x[use] * w[use, None])
    filled = mass > 0
    c[filled] = sums[filled] / mass[filled, None]
    return c, mass


def case(P, K, D, kind, seed=0):
    """rows [P,D], codebook [K,D] fp32 (torch): normal, shifted by KINDS[kind] in every dimension."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * P + 3 * K + D)
    off = KINDS[kind]
    return (torch.randn(P, D, generator=g) + off).float(), (torch.randn(K, D, generator=g) + off).float()


def planted(P, K, D, seed=0, spread=0.05, scale=8.0):
    """Well-separated blobs: -> rows [P,D], label [P], init [K,D] (one row of every blob).  Centre k sits on axis k mod D at scale (1 + k // D): any two are at least
    `scale` apart while a blob's radius is a few `spread`."""
    g = torch.Generator().manual_seed(5000 + seed)
    centres = torch.zeros(K, D)
    for k in range(K):
        centres[k, k % D] = scale * (1 + k // D)
    label = torch.arange(P) % K
    label = label[torch.randperm(P, generator=g)]
    rows = (centres[label] + spread * torch.randn(P, D, generator=g)).float()
    first = torch.stack([torch.nonzero(label == k)[0, 0] for k in range(K)])
    return rows, label.to(torch.int32), rows[first].clone()


def check_assign(tag, rows, codebook, idx, dist2):
    """The assignment bar and the dist2 bar on clean data (every row and at least one centroid finite)."""
    x, c = rows.double().numpy(), codebook.double().numpy()
    P, D = x.shape
    idx, dist2 = np.asarray(idx), np.asarray(dist2, dtype=np.float64)
    assert idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < c.shape[0], (tag, idx.min(), idx.max())
    want, best = assign64(x, c)
    got = ((x - c[idx]) ** 2).sum(axis=1)
    slack = gamma(D) * ((x * x).sum(axis=1) + (c[idx] ** 2).sum(axis=1) + (c[want] ** 2).sum(axis=1))
    worst = float(((got - best) / np.maximum(slack, 1e-300)).max())
    print(f"[{tag}] assign: {int((idx != want).sum())} of {P} rows differ from the fp64 argmin, worst excess {worst:.3g} of the bar")
    assert (got <= best + slack).all(), (tag, worst)
    rel = float((np.abs(dist2 - got) / np.maximum(got, 1e-300)).max()) if P else 0.0
    print(f"[{tag}] dist2: worst relative error {rel:.3g} (bar {dist2_bar(D):.3g})")
    assert (np.abs(dist2 - got) <= dist2_bar(D) * got).all(), (tag, rel)
    return want


def check_update(tag, rows, weights, idx, codebook_in, codebook_out, mass):
    x = rows.double().numpy()
    want_c, want_m = update64(x, None if weights is None else weights.numpy(), idx, codebook_in.double().numpy())
    got_c, got_m = codebook_out.double().numpy(), np.asarray(mass, dtype=np.float64)
    empty = want_m == 0
    assert np.array_equal(codebook_out.numpy().view(np.int32)[empty], codebook_in.numpy().view(np.int32)[empty]), (tag, "an empty cluster moved")
    assert (got_m[empty] == 0).all(), tag
    err_c = np.abs(got_c - want_c)[~empty] / ulp32(want_c[~empty])
    err_m = np.abs(got_m - want_m)[~empty] / ulp32(want_m[~empty])
    print(f"[{tag}] update: {int((~empty).sum())} filled clusters, worst centroid error {float(err_c.max()) if err_c.size else 0:.3g} ulp, "
          f"mass {float(err_m.max()) if err_m.size else 0:.3g} ulp")
    assert (err_c <= 1.0).all() and (err_m <= 1.0).all(), tag


def lloyd_step_tolerance(rows, weights, codebook, idx, inertia_before, inertia_after):
    """What the kernel's inertia of the assignment `idx` to `codebook` may exceed the inertia of the assignment before it by, when `codebook` holds
    the fp32 weighted means of that earlier assignment A (all fp64 here; rows with idx -1 carry no bar).  With J(A, C) = sum w |x - c_A(p)|^2:
      J(A, means) <= J(A, C_before)                                   the mean minimises a cluster's weighted squared distances;
      J(A, rounded means) = J(A, means) + sum_k mass_k |delta_k|^2    exactly, and |delta_kd| <= ulp32(c_kd), the update's bar;
      J(idx, C) <= J(A, C) + sum w slack_p                            row by row: the assignment bar against the fp64 best, which is no farther than A's;
    and either reported inertia is within dist2's relative bar of its fp64 value."""
    x, c = np.asarray(rows, dtype=np.float64), np.asarray(codebook, dtype=np.float64)
    D = x.shape[1]
    w = clean_weights(weights, x.shape[0])
    idx = np.asarray(idx)
    ok = idx >= 0
    want, _ = assign64(x[ok], c)
    slack = gamma(D) * ((x[ok] ** 2).sum(axis=1) + (c[idx[ok]] ** 2).sum(axis=1) + (c[want] ** 2).sum(axis=1))
    rounding = float(w[ok].sum()) * float((ulp32(c) ** 2).sum(axis=1).max())
    return float((w[ok] * slack).sum()) + rounding + dist2_bar(D) * (float(inertia_before) + float(inertia_after))
