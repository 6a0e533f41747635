"""Times the candidate lists of identities (fn_gallery_candidates) against fn_gallery_search at the same k
and against the route a user had before: search(k = 64) and removing duplicate labels on the host.  E = 512, k = 5, tight
synthetic classes (the generator of tools/bench_cluster.py) stored class after class, as class directories are:

  (a) Q = 16 faces against G = 1 048 576 rows in classes of 16 contiguous rows;
  (b) leave-one-out over Q = G = 26 495 rows in 530 contiguous classes of about 50 (skip = the row itself): a probe's own
      identity has dozens of rows below the threshold of the k-th DISTINCT identity, the shape that makes the cut run most;
  (c) the rows of (b) with labels = arange: every row its own identity, the selection work of fn_gallery_search.

In one process, alternating, per shape:

  search          Gallery._search(k = 5, atol=None): fn_gallery_search, nothing read back;
  candidates      Gallery._candidates(k = 5, atol=None): fn_gallery_candidates, nothing read back;
  search64+host   Gallery._search(k = 64), both arrays copied to the host, the first 5 distinct labels of every row kept there.

Also reported: whether the candidates equal the host route wherever that route found 5 identities, the share of probes whose 64
nearest rows hold fewer than 5 identities (for which that route has no answer), and for (c) whether the candidates are the
search's arrays bit for bit.  Every sample is a device-event window (which also spans the host work between its two records)
around enough back-to-back calls to last about 20 ms, after a warm-up of every path; median of --reps.  Prints readable lines
and, last, one JSON line; --out also writes them to a file.

    python tools/bench_candidates.py [--reps 7] [--shapes abc] [--out profiles/candidates_bench.txt]"""
import argparse, json, sys
import numpy as np, torch
sys.path.insert(0, ".")
from facenet_amd.recognize import Gallery

E, K, WIDE = 512, 5, 64
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--shapes", default="abc")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


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


def class_rows(labels, gen):
    """Unit rows, row i a member of the tight class labels[i]."""
    classes = int(labels.max().item()) + 1
    centres = unit(torch.randn(classes, E, device=dev, generator=gen))
    out = torch.empty(len(labels), E, device=dev)
    for lo in range(0, len(labels), 1 << 16):                  # in pieces: the noise of a million rows is 2 GiB
        part = labels[lo:lo + (1 << 16)]
        out[lo:lo + len(part)] = unit(centres[part] + 0.3 * torch.randn(len(part), E, device=dev, generator=gen) / E ** 0.5)
    return out


def distinct_on_host(gallery, queries, skip):
    """The route without fn_gallery_candidates -> (rows int32 [Q, K] of the first K distinct labels among the 64 nearest rows, -1
    where there are fewer; the number of distinct labels found per probe)."""
    dist, rows = (t.cpu().numpy() for t in gallery._search(queries, WIDE, skip, 0, None))
    found = np.where(rows >= 0, gallery.labels[np.maximum(rows, 0)], -1)
    first = rows >= 0
    for j in range(1, WIDE):
        first[:, j] &= (found[:, :j] != found[:, j:j + 1]).all(axis=1)
    order = np.argsort(~first, axis=1, kind="stable")[:, :K]      # the first occurrences, in their order
    kept = np.take_along_axis(first, order, axis=1)
    return np.where(kept, np.take_along_axis(rows, order, axis=1), -1).astype(np.int32), first.sum(axis=1)


def run(shape):
    gen = torch.Generator(device=dev).manual_seed(1)
    if shape == "a":
        G, Q = 1 << 20, 16
        labels = torch.arange(G, device=dev) // 16
        rows = class_rows(labels, gen)
        queries = unit(rows[torch.arange(Q, device=dev) * 65521 % G] + 0.3 * torch.randn(Q, E, device=dev, generator=gen) / E ** 0.5).contiguous()
        skip = None
    else:
        G = Q = 26495
        labels = torch.arange(G, device=dev) * 530 // G
        rows = class_rows(labels, gen)
        queries, skip = rows, np.arange(G, dtype=np.int32)
    host_labels = np.arange(G) if shape == "c" else labels.cpu().numpy()
    gallery = Gallery(rows, labels=host_labels, device=dev)
    gallery._label_codes()
    torch.cuda.synchronize()
    paths = {"search": lambda: gallery._search(queries, K, skip, 0, None),
             "candidates": lambda: gallery._candidates(queries, K, skip, 0, None),
             "search64+host": lambda: distinct_on_host(gallery, queries, skip)}
    t = bench(paths, args.reps)
    got = gallery._candidates(queries, K, skip, 0, None)
    host_rows, host_found = distinct_on_host(gallery, queries, skip)
    complete = host_found >= K
    out = {"shape": shape, "Q": Q, "G": G, "E": E, "k": K, "classes": int(len(np.unique(host_labels))),
           **{name: stats(v) for name, v in t.items()},
           "candidates_over_search": round(float(np.median(t["candidates"]) / np.median(t["search"])), 3),
           "host_route_over_candidates": round(float(np.median(t["search64+host"]) / np.median(t["candidates"])), 3),
           "probes_with_fewer_than_k_identities_in_64_rows": round(float((~complete).mean()), 6),
           "equals_host_route_where_complete": bool(np.array_equal(got[1].cpu().numpy()[complete], host_rows[complete]))}
    if shape == "c":
        want = gallery._search(queries, K, skip, 0, None)
        out["equals_search_bit_for_bit"] = bool(torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]))
    say(f"({shape}) Q {Q} G {G} in {out['classes']} classes: search {out['search']['median_ms']} ms, candidates "
        f"{out['candidates']['median_ms']} ms ({out['candidates_over_search']} x the search), search(k=64) + host "
        f"{out['search64+host']['median_ms']} ms ({out['host_route_over_candidates']} x the candidates)")
    say(f"    probes whose 64 nearest rows hold fewer than {K} identities: {out['probes_with_fewer_than_k_identities_in_64_rows']}; "
        f"candidates == host route where that is complete: {out['equals_host_route_where_complete']}"
        + (f"; candidates == search bit for bit: {out['equals_search_bit_for_bit']}" if shape == "c" else ""))
    return out


results = [run(shape) for shape in args.shapes]
ok = all(r["equals_host_route_where_complete"] and r.get("equals_search_bit_for_bit", True) for r in results)
say(json.dumps({"bench": "candidates", "device": torch.cuda.get_device_name(0), "reps": args.reps, "results": results, "all_equal": ok}))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(0 if ok else 1)
