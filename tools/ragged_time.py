"""Ragged batch timing probe (development aid).

    ragged_time.py [--blocks B] [--steps S] [--repeats R] [--warmup W]

(a) uniform: B blocks (default 65536) of 16 cities in f64, the bench's
    instance (`./tsp 16 B 1000 1000`).  tspgpu_solve_ragged_device against
    tspgpu_solve_blocks_device on the same device buffer: what the gather, the
    scatter and the descriptor upload add to the solve.
(b) mixed: B blocks with sizes uniform over 8..16 (--sizes), in random order.  The
    ragged call against the same blocks grouped by hand into one contiguous
    array per size and one tspgpu_solve_blocks_device call per size (the
    host-side sort and the putting back in order are NOT in the hand-grouped
    time: it is the floor).

Every time is a pair of HIP events on the context's stream around S calls
(after W untimed warm-up calls of each path), repeated R times with the two
paths alternating; the median, min and max of the per-call time over the
repeats are reported, and a last line of JSON.  The answers of the two paths
are compared bit for bit before anything is timed."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tsp-mpi-reduction_amd"), ROOT]
import numpy as np
import tspgpu
from bench import Shard  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=65536)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--sizes", type=int, nargs=2, default=[8, 16], metavar=("LO", "HI"), help="(b): sizes LO..HI")
args = ap.parse_args()
B = args.blocks

ctx = tspgpu.Context(device=0)
cu, name = ctx.device_info()
print(f"device: {name}; blocks={B} steps={args.steps} repeats={args.repeats} warmup={args.warmup}", flush=True)


def timed(paths):
    """paths: {label: callable enqueueing one call on ctx.stream} -> {label: [ms per call] * repeats}"""
    for fn in paths.values():
        for _ in range(args.warmup):
            fn()
    ctx.synchronize()
    out = {k: [] for k in paths}
    for _ in range(args.repeats):
        for label, fn in paths.items():  # alternating
            ctx.timer_start()
            for _ in range(args.steps):
                fn()
            out[label].append(ctx.timer_stop() / args.steps)
    return out


def summary(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)),
            "repeats_ms": [round(float(x), 3) for x in ms]}


def show(case, label, s):
    print(f"{case} {label:<28} median={s['median_ms']:.3f} ms min={s['min_ms']:.3f} max={s['max_ms']:.3f} "
          f"(of {args.repeats} x {args.steps} calls: {' '.join(f'{x:.2f}' for x in s['repeats_ms'])})", flush=True)


result = {"blocks": B, "steps": args.steps, "repeats": args.repeats, "device": name}

# (a) uniform ------------------------------------------------------------------------------------
n = 16
d = Shard(n, B, 0, B).distances()
dd = ctx.upload(d)
c_u, t_u = ctx.alloc(B * 8), ctx.upload(np.full((B, n + 1), -1, dtype=np.int32))
c_r, t_r, s_r = ctx.alloc(B * 8), ctx.alloc(B * (n + 1) * 4), ctx.alloc(B * 4)
off = np.arange(B, dtype=np.int64) * (n * n)
ns = np.full(B, n, dtype=np.int32)


def uniform():
    ctx.solve_device(dd, n, B, c_u, t_u, ctx.stream)


def ragged_uniform():
    ctx.solve_ragged_device(dd, tspgpu.F64, off, ns, c_r, t_r, n + 1, s_r, ctx.stream)


uniform(); ragged_uniform(); ctx.synchronize()
variant = ctx.last_variant()
assert not ctx.download(s_r, (B,), np.int32).any()
assert np.array_equal(ctx.download(c_u, (B,), np.uint64), ctx.download(c_r, (B,), np.uint64))
assert np.array_equal(ctx.download(t_u, (B, n + 1), np.int32), ctx.download(t_r, (B, n + 1), np.int32))
t = timed({"solve_device": uniform, "solve_ragged_device": ragged_uniform})
a = {k: summary(v) for k, v in t.items()}
a["difference_ms"] = a["solve_ragged_device"]["median_ms"] - a["solve_device"]["median_ms"]
a["variant"] = variant
# the bytes the two extra passes move: the matrices read and written once by the gather (K1
# then reads the bucket instead of the caller's array: nothing extra), per block the 32-byte
# descriptor in both passes, the status written, read and written, the cost and the tour read
# and written
a["gather_scatter_bytes"] = 2 * d.nbytes + B * (32 + 32 + 4 + 4 + 2 * 8 + 2 * (n + 1) * 4 + 4)
for k in ("solve_device", "solve_ragged_device"):
    show("(a) uniform n=16", k, a[k])
print(f"(a) uniform n=16 difference = {a['difference_ms']:.3f} ms "
      f"({100 * a['difference_ms'] / a['solve_device']['median_ms']:.1f}% of the solve; K1 variant {variant}; "
      f"gather + scatter move {a['gather_scatter_bytes'] / 1e6:.0f} MB)", flush=True)
result["uniform"] = a
for p in (dd, c_u, t_u, c_r, t_r, s_r):
    ctx.free(p)

# (b) mixed --------------------------------------------------------------------------------------
rng = np.random.default_rng(2027)
LO, HI = args.sizes
sizes = rng.integers(LO, HI + 1, B).astype(np.int32)
per = {}
for k in range(LO, HI + 1):
    cnt = int((sizes == k).sum())
    per[k] = Shard(k, cnt, 0, cnt).distances() if cnt else np.zeros((0, k, k))
# caller order: block b is the next unused block of its size
taken = {k: 0 for k in per}
off = np.zeros(B, dtype=np.int64)
pieces, at = [], 0
for b in range(B):
    k = int(sizes[b])
    pieces.append(per[k][taken[k]].ravel())
    taken[k] += 1
    off[b] = at
    at += k * k
flat = np.concatenate(pieces) if pieces else np.zeros(0)
d_flat = ctx.upload(flat)
c_r, t_r, s_r = ctx.alloc(B * 8), ctx.alloc(B * (HI + 1) * 4), ctx.alloc(B * 4)
hand = {k: (ctx.upload(m), m.shape[0], ctx.alloc(max(1, m.shape[0]) * 8),
            ctx.upload(np.full((max(1, m.shape[0]), k + 1), -1, dtype=np.int32))) for k, m in per.items()}


def grouped():
    for k, (pd, cnt, pc, pt) in hand.items():
        if cnt:
            ctx.solve_device(pd, k, cnt, pc, pt, ctx.stream)


def ragged_mixed():
    ctx.solve_ragged_device(d_flat, tspgpu.F64, off, sizes, c_r, t_r, HI + 1, s_r, ctx.stream)


grouped(); ragged_mixed(); ctx.synchronize()
assert not ctx.download(s_r, (B,), np.int32).any()
cost_r, tour_r = ctx.download(c_r, (B,), np.uint64), ctx.download(t_r, (B, HI + 1), np.int32)
for k, (pd, cnt, pc, pt) in hand.items():
    if cnt:
        idx = np.flatnonzero(sizes == k)
        assert np.array_equal(ctx.download(pc, (cnt,), np.uint64), cost_r[idx]), k
        assert np.array_equal(ctx.download(pt, (cnt, k + 1), np.int32), tour_r[idx, :k + 1]), k
        assert (tour_r[idx, k + 1:] == -1).all(), k
t = timed({"solve_device per size": grouped, "solve_ragged_device": ragged_mixed})
m = {k: summary(v) for k, v in t.items()}
m["difference_ms"] = m["solve_ragged_device"]["median_ms"] - m["solve_device per size"]["median_ms"]
m["blocks_per_size"] = {str(k): int(v[1]) for k, v in hand.items()}
for k in ("solve_device per size", "solve_ragged_device"):
    show(f"(b) mixed n={LO}..{HI}", k, m[k])
print(f"(b) mixed n={LO}..{HI} difference = {m['difference_ms']:.3f} ms "
      f"({100 * m['difference_ms'] / m['solve_device per size']['median_ms']:.1f}% of the hand-grouped solves)",
      flush=True)
result["mixed"] = m
print(json.dumps(result))
