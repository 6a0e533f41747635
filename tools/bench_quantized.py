"""Times the quantised gallery (fn_quantize_rows / fn_qgallery_search) against the exhaustive
fn_gallery_search at the two shapes of section 19, k = 5, E = 512:

  (A) Q = 16 faces against G = 1 048 576 known faces;
  (B) leave-one-out over Q = G = 26 495 rows (skip = the row itself),

each on unit-norm random rows and on tight synthetic classes (the generator of tools/bench_cluster.py: (A) 20 000 classes, the
queries further members; (B) 530 classes).  In one process, alternating, per shape and data set:

  exhaustive      Gallery._search (atol=None): fn_gallery_search and its workspace from the caching allocator;
  approx R        QuantizedGallery._search(shortlist=R, exact=False, atol=None) for R = 16, 32, 64: the queries' quantisation, the
                  shortlist and the re-rank, nothing read back;
  exact R         the same with exact=True: the certificate read back and the uncertified queries run through fn_gallery_search.

Also reported: the share of queries certified, whether the exact result equals the exhaustive one bit for bit, recall@5 of the
approximate result, and the time to quantise the gallery.  Every sample is a device-event window (which also spans the host work
between its two records) around enough back-to-back calls to last about 20 ms, after a warm-up of every path; median of --reps.
Prints readable lines and, last, one JSON line.

    python tools/bench_quantized.py [--reps 7] [--shapes AB]"""
import argparse, json, sys
import numpy as np, torch
sys.path.insert(0, ".")
from facenet_amd.recognize import Gallery

E, K = 512, 5
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--shapes", default="AB")
args = ap.parse_args()
dev = torch.device("cuda:0")


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / inner


def bench(paths, reps):
    inner = {}
    for name, fn in paths.items():
        window(fn, 2)
        inner[name] = max(1, min(200, int(0.02 / max(window(fn, 1), 1e-6))))
    samples = {name: [] for name in paths}
    for _ in range(reps):
        for name, fn in paths.items():
            samples[name].append(window(fn, inner[name]))
    return {name: np.array(v) for name, v in samples.items()}


def stats(t):
    return {"median_ms": round(float(np.median(t)) * 1e3, 4), "min_ms": round(float(t.min()) * 1e3, 4), "max_ms": round(float(t.max()) * 1e3, 4)}


unit = lambda x: x / x.norm(dim=1, keepdim=True)


def rows_of(n, classes, gen):
    """n unit rows: random (classes None), or members of ``classes`` tight classes (tools/bench_cluster.py)."""
    if classes is None:
        return unit(torch.randn(n, E, device=dev, generator=gen)).contiguous()
    centres = unit(torch.randn(classes, E, device=dev, generator=gen))
    return unit(centres[torch.arange(n, device=dev) % classes] + 0.3 * torch.randn(n, E, device=dev, generator=gen) / E ** 0.5).contiguous()


def run(shape, data):
    gen = torch.Generator(device=dev).manual_seed(1)
    if shape == "A":
        G, Q, classes = 1 << 20, 16, 20000 if data == "classes" else None
        pool = rows_of(G + Q, classes, gen)
        rows, queries, skip = pool[:G].contiguous(), pool[G:].contiguous(), None
    else:
        G = Q = 26495
        rows = rows_of(G, 530 if data == "classes" else None, gen)
        queries, skip = rows, np.arange(G, dtype=np.int32)
    gallery = Gallery(rows, device=dev)
    qg = gallery.quantize()
    torch.cuda.synchronize()
    from facenet_amd.quantized import quantize_rows
    t_quant = stats(bench({"q": lambda: quantize_rows(rows)}, args.reps)["q"])
    paths = {"exhaustive": lambda: gallery._search(queries, K, skip, 0, None)}
    for R in (16, 32, 64):
        paths[f"approx {R}"] = lambda R=R: qg._search(queries, K, skip, 0, None, shortlist=R, exact=False)
        paths[f"exact {R}"] = lambda R=R: qg._search(queries, K, skip, 0, None, shortlist=R, exact=True)
    t = bench(paths, args.reps)
    want = gallery._search(queries, K, skip, 0, None)
    out = {"shape": shape, "data": data, "Q": Q, "G": G, "E": E, "k": K, "quantize_gallery": t_quant, "exhaustive": stats(t["exhaustive"])}
    base = float(np.median(t["exhaustive"]))
    for R in (16, 32, 64):
        dist, near, cert = qg._certified_search(queries, K, skip, 0, None, R)
        exact = qg._search(queries, K, skip, 0, None, shortlist=R, exact=True)
        hits = (near.unsqueeze(2) == want[1].unsqueeze(1)).any(dim=2).float().mean().item()
        out[f"shortlist {R}"] = {"approx": stats(t[f"approx {R}"]), "exact": stats(t[f"exact {R}"]),
                                 "approx_speedup": round(base / float(np.median(t[f"approx {R}"])), 3),
                                 "exact_speedup": round(base / float(np.median(t[f"exact {R}"])), 3),
                                 "certified_share": round(float((cert != 0).float().mean().item()), 6), "fallbacks": qg.last_fallbacks,
                                 "recall_at_5_of_approx": round(hits, 6),
                                 "exact_equals_exhaustive": bool(torch.equal(exact[0], want[0]) and torch.equal(exact[1], want[1])),
                                 "certified_rows_equal_exhaustive": bool(torch.equal(near[cert != 0], want[1][cert != 0]))}
    print(f"({shape}) {data}: Q {Q} G {G}; quantise the gallery {t_quant['median_ms']} ms; exhaustive {out['exhaustive']['median_ms']} ms", flush=True)
    for R in (16, 32, 64):
        r = out[f"shortlist {R}"]
        print(f"    shortlist {R:2d}: approx {r['approx']['median_ms']} ms ({r['approx_speedup']} x), exact {r['exact']['median_ms']} ms "
              f"({r['exact_speedup']} x), certified {r['certified_share']}, recall@5 of approx {r['recall_at_5_of_approx']}, "
              f"exact == exhaustive {r['exact_equals_exhaustive']}", flush=True)
    return out


results = [run(shape, data) for shape in args.shapes for data in ("random", "classes")]
ok = all(r[f"shortlist {R}"]["exact_equals_exhaustive"] and r[f"shortlist {R}"]["certified_rows_equal_exhaustive"] for r in results for R in (16, 32, 64))
print(json.dumps({"bench": "quantized", "device": torch.cuda.get_device_name(0), "reps": args.reps, "results": results, "all_exact": ok}))
sys.exit(0 if ok else 1)
