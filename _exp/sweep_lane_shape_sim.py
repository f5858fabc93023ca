"""Pruned C2 sweep, offline model (r07): which (wave, chunk) and (block, chunk) combinations the
box bound  min D32 + min W32 <= thr  leaves live, per shape of the wave's sources x destinations.

A wave runs a 32-row chunk if ANY of its pairs (source s, destination t) can pass the bound
minD[s][c] + minW[c][t] <= thr(t, s); a block stages the chunk if any of its waves runs it.  The
bound is symmetric in D and W, so the wave may hold 64 sources x 8 destinations (the source-lane
chunk loop, k_relax_dense_f) or 8 sources x 64 destinations (k_sweep_dest_lanes), or anything
between.  The model:
  * the C2 generator (synth.geometric_complete_ish) at V vertices, V / 10 attached;
  * the vertices in a Hilbert order of their true coordinates (the engine's locality order is a
    landmark embedding of the same plane);
  * the attached vertices in that order, 64 per batch;
  * thresholds = the distances after two min-plus rounds from the direct arcs (the final ones on
    C2 to within the rounds the engine itself needs);
  * minD = per-chunk minima of the direct-arc rows (the state the first sweep reads), minW = the
    per-chunk, per-column minima of W.
Thresholds only fall during a sweep, so the final ones give the floor of each shape's work.
usage: python3 _exp/sweep_lane_shape_sim.py [V] [batch indices, comma separated]
"""
import sys

import numpy as np

sys.path.insert(0, ".")
from shadow_amd import synth  # noqa: E402

V = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000
A = V // 10
SRS, KL = 32, 64
nb = (A + KL - 1) // KL
BATCHES = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else sorted({0, nb // 2, nb - 2 if nb > 2 else nb - 1})


def hilbert(x, y, n=1 << 12):
    x = (x * (n - 1)).astype(np.int64)
    y = (y * (n - 1)).astype(np.int64)
    dd = np.zeros_like(x)
    s = n >> 1
    while s > 0:
        rx = ((x & s) > 0).astype(np.int64)
        ry = ((y & s) > 0).astype(np.int64)
        dd += s * s * ((3 * rx) ^ ry)
        m = ry == 0
        f = m & (rx == 1)
        x = np.where(f, n - 1 - x, x)
        y = np.where(f, n - 1 - y, y)
        x2 = np.where(m, y, x)
        y = np.where(m, x, y)
        x = x2
        s >>= 1
    return dd


g = synth.geometric_complete_ish(V=V, A=A)
pts = np.random.default_rng(1).random((V, 2))  # the generator's first draw: the true coordinates
perm = np.argsort(hilbert(pts[:, 0], pts[:, 1]), kind="stable")
pos = np.empty(V, np.int64)
pos[perm] = np.arange(V)
# dense W in the order (rows = tails u, columns = heads t), +inf where there is no arc; loops dropped
W = np.full((V, V), np.inf, np.float32)
src, dst = pos[np.asarray(g.src)], pos[np.asarray(g.dst)]
lat = np.asarray(g.latency, np.float32)
keep = src != dst
W[src[keep], dst[keep]] = lat[keep]  # (the generator has no parallel arcs)
if not g.directed:
    W = np.minimum(W, W.T)
att = np.sort(pos[np.asarray(g.attached)])  # attached vertices as positions, in the order
nchunks = (V + SRS - 1) // SRS
Vc = nchunks * SRS
Vt = (V + KL - 1) // KL * KL  # destinations padded to whole 64-tiles (padding never passes)
Wr = np.full((Vc, V), np.inf, np.float32)
Wr[:V] = W
minW = Wr.reshape(nchunks, SRS, V).min(1)  # [chunk][t]
del Wr


def min_plus(D):
    """out[s][t] = min(D[s][t], min_u D[s][u] + W[u][t]), rows of u in blocks"""
    out = D.copy()
    tmp = np.empty((1024, V), np.float32)
    for s in range(D.shape[0]):
        for u0 in range(0, V, 1024):
            n = min(1024, V - u0)
            np.add(W[u0:u0 + n], D[s, u0:u0 + n, None], out=tmp[:n])
            np.minimum(out[s], tmp[:n].min(0), out=out[s])
    return out


SHAPES = [("wave 64 x 8, block 64 x 32 (source lanes)", 64, 8, 64, 32),
          ("wave 8 x 64, block 32 x 64 (destination lanes)", 8, 64, 32, 64),
          ("wave 16 x 32", 16, 32, None, None),
          ("wave 32 x 16", 32, 16, None, None),
          ("single pairs (floor of any box bound)", 1, 1, None, None)]
acc = {name: [0, 0, 0, 0] for name, *_ in SHAPES}  # live waves, wave slots, live blocks, block slots
for b in BATCHES:
    S = att[b * KL:(b + 1) * KL]
    ns = len(S)
    D0 = np.full((KL, V), np.inf, np.float32)
    D0[:ns] = W[S]                      # the direct arcs (the seeded state)
    thr = D0.copy()
    thr[np.arange(ns), S] = 0.0
    thr = min_plus(min_plus(thr))
    thr[np.arange(ns), S] = -np.inf     # a source's own pair is never relaxed
    thr[ns:] = -np.inf                  # slots without a source never pass
    D0r = np.full((KL, Vc), np.inf, np.float32)
    D0r[:, :V] = D0
    minD = D0r.reshape(KL, nchunks, SRS).min(2)  # [s][chunk]
    thr_p = np.full((KL, Vt), -np.inf, np.float32)
    thr_p[:, :V] = thr * np.float32(1 + 1e-6)
    minW_p = np.full((nchunks, Vt), np.inf, np.float32)
    minW_p[:, :V] = minW
    live = np.empty((nchunks, KL, Vt), bool)
    for c in range(nchunks):
        live[c] = minD[:, c, None] + minW_p[c][None, :] <= thr_p
    ntiles = {gt: (V + gt - 1) // gt for gt in (1, 8, 16, 32, 64)}
    for name, gs, gt, bs, bt in SHAPES:
        w = live.reshape(nchunks, KL // gs, gs, Vt // gt, gt).any(axis=(2, 4))[:, :, :ntiles[gt]]
        acc[name][0] += int(w.sum())
        acc[name][1] += w.size
        if bs:
            bl = live.reshape(nchunks, KL // bs, bs, Vt // bt, bt).any(axis=(2, 4))[:, :, :ntiles[bt]]
            acc[name][2] += int(bl.sum())
            acc[name][3] += bl.size
    print(f"batch {b}: {ns} sources done", file=sys.stderr, flush=True)

print(f"C2 generator, V = {V}, A = {A}, batches {BATCHES} of {nb}, every tile, {nchunks} chunks of {SRS} rows")
print(f"{'shape (sources x destinations)':50s} {'live (wave, chunk)':>19s} {'live (block, chunk)':>20s} {'waves per staged chunk':>23s}")
for name, *_ in SHAPES:
    lw, sw, lb, sb = acc[name]
    fw = lw / sw
    if sb:
        print(f"{name:50s} {fw:19.3f} {lb / sb:20.3f} {fw / (lb / sb):23.2f}")
    else:
        print(f"{name:50s} {fw:19.3f}")
