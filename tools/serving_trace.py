"""Host and device timeline of the serving loop, ticket by ticket (no profiler attached).

COOCC_SERVING_TRACE=1 python tools/serving_trace.py [config] [frames] [slots] [dense_streams] [ahead]
Device times from HIP events (time_dense), host times from perf_counter, both relative to one synchronised origin.
"""
import os
import sys
import time

os.environ["COOCC_SERVING_TRACE"] = "1"
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import bench  # noqa: E402
from co_occ_amd import serving, streams  # noqa: E402


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "r50"
    nfr = int(sys.argv[2]) if len(sys.argv) > 2 else 36
    slots = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    nds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    ahead = int(sys.argv[5]) if len(sys.argv) > 5 else 0
    dev = torch.device("cuda:0")
    model, _ = bench.build_model(cfg, dev)
    samples = [bench.make_inputs(cfg, 1234 + i, dev, model) for i in range(slots)]
    frames = [bench.frame_of(x) for x in samples]
    gp = model.serving(frames[0], slots=slots, dense_streams=nds, ahead=ahead)
    gp.run(frames, 2 * slots)
    gp.time_dense = True
    gp.run(frames, slots)
    torch.cuda.synchronize()
    gp.trace.clear()
    gp.dense_ev.clear()
    base = streams.new_event(timing=True)      # the type of Ticket.events / dense_ev: elapsed_time() needs both ends alike
    base.record()
    base.synchronize()
    h0 = time.perf_counter()
    first = gp._submitted
    gp.run(frames, nfr)
    torch.cuda.synchronize()
    wall = time.perf_counter() - h0
    print("%s: %d frames, slots %d, dense streams %d, searches ahead %d: %.3f ms per frame" % (cfg, nfr, slots, nds, gp.ahead, 1e3 * wall / nfr))
    host = {}
    for idx, tag, ts in gp.trace:
        host.setdefault(idx, {})[tag] = 1e3 * (ts - h0)
    print("ticket | host: dispatch  search_begin  native_call  search_end  issue_begin  issue_end | device: search start..end   dense start..end")
    for e0, e1, idx, sev in gp.dense_ev:
        h = host.get(idx, {})
        g = lambda k: "%8.2f" % h[k] if k in h else "    --  "
        s0, s1 = (base.elapsed_time(sev[0]), base.elapsed_time(sev[1])) if sev else (float("nan"),) * 2
        print("%5d  | %s %s %s %s %s %s | %8.2f .. %8.2f   %8.2f .. %8.2f  (%.2f)" % (
            idx - first, g("dispatch"), g("search_begin"), g("search_native"), g("search_end"), g("issue_begin"), g("issue_end"),
            s0, s1, base.elapsed_time(e0), base.elapsed_time(e1), e0.elapsed_time(e1)))
    summary(gp, base, wall)


def summary(gp, base, wall):
    """What the table above says about the schedule: spans of the two stages, how long a dense stream idles between two replays and
    what share of the window its replays fill, and how many launches carry a frame's dense-stage inputs into its slot."""
    med = lambda v: sorted(v)[len(v) // 2] if v else float("nan")
    line = lambda name, v: print("%-72s: median %.2f  min %.2f  max %.2f" % (name, med(v), min(v), max(v)))
    lanes = getattr(gp, "lanes", False)
    print("search stage on %s" % ("its slot's dense stream (lanes)" if lanes else "a stream of its own per slot"))
    line("device span of the search stage (Ticket.events), ms", [sev[0].elapsed_time(sev[1]) for _, _, _, sev in gp.dense_ev if sev])
    line("dense span (events around the replay), ms", [e0.elapsed_time(e1) for e0, e1, _, _ in gp.dense_ev])
    per, gaps, busy = {}, [], 0.0
    for e0, e1, idx, sev in gp.dense_ev:
        per.setdefault(idx % gp.n % gp.ndense, []).append((base.elapsed_time(e0), base.elapsed_time(e1), sev))
    for k, v in sorted(per.items()):
        busy += sum(b - a for a, b, _ in v)
        gaps += [v[i + 1][0] - v[i][1] for i in range(len(v) - 1)]
    line("idle gap of a dense stream between two replays, ms", gaps)
    if lanes:        # the search of the next ticket sits in that gap: what of it is neither search nor replay
        rest = []
        for v in per.values():
            rest += [v[i + 1][0] - v[i][1] - v[i + 1][2][0].elapsed_time(v[i + 1][2][1]) for i in range(len(v) - 1) if v[i + 1][2]]
        line("... of which not the lane's own search stage, ms", rest)
    print("dense streams busy over the window: %.1f ms of replays / (%d x %.1f ms) = %.0f %%" % (
        busy, gp.ndense, 1e3 * wall, 100 * busy / (gp.ndense * 1e3 * wall)))
    tab = getattr(gp, "_copy_tables", [None])[0]
    st = gp.static[0]
    ntens = 1 + len(st["cams"] or ()) + sum(torch.is_tensor(t) for t in st["transform"][:-1]) + (st["gemo"] is not None)
    nl = ntens if tab is None or not getattr(serving, "COPY_MANY", False) else -(-len(tab) // 16)
    print("dense-stage inputs of a frame: %d tensors copied into the slot by %d launch%s" % (ntens, nl, "" if nl == 1 else "es"))


if __name__ == "__main__":
    main()
