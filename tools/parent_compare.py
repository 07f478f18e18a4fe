"""What the parent-comparison tools (conv_vs_parent.py, wgrad_vs_parent.py) share: a second build of the library loaded into the
same process and swapped under ops.*, the NaN-aware equality of NaN-prefilled outputs, and the alternated timing rounds with
the parent against itself as the yardstick."""
import ctypes, importlib.util, json, os, statistics, sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sdeflow_light_amd import _lib  # noqa: E402


def load(path):
    return _lib.bind(ctypes.CDLL(os.path.abspath(path)), missing_ok=True)     # an entry this tree added is missing from the other build


def use(h):
    _lib._lib = h                       # ops.* resolves the library through _lib.lib()


def test_module(name):
    """tests/<name>.py as a module (the tools take their shapes from the tests, not from copies of them)."""
    if os.path.join(ROOT, "tests") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def same(a, b):
    """Bitwise equality of two outputs that started NaN-filled: every element either build writes is finite, NaN marks what
    neither wrote and must sit at the same places (a skipped store shows)."""
    if a is None or b is None:
        return a is None and b is None
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def timed_rounds(call, parent, builds, rounds, reps, warm):
    """rounds + 1 rounds of (parent, parent again, then every (name, library) of builds), each the median of reps event-timed
    call(library) after warm untimed ones; the first round is a warm-up and is dropped.  The yardstick is the parent against
    itself: pp = the largest |parent - parent again| of one round.  A build holds when |its median - the parent's median| <= pp;
    beyond that it is faster or SLOWER.  Returns the row that goes into the JSON (microseconds)."""
    def med(h):
        for _ in range(warm):
            call(h)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record(); call(h); b.record()
        torch.cuda.synchronize()
        return statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3
    p1, p2, t = [], [], {n: [] for n, _ in builds}
    for r in range(rounds + 1):
        x1, x2 = med(parent), med(parent)
        xs = [med(h) for _, h in builds]
        if r:
            p1.append(x1); p2.append(x2)
            for (n, _), x in zip(builds, xs):
                t[n].append(x)
    mp = statistics.median(p1 + p2)
    pp = max(abs(a - b) for a, b in zip(p1, p2))
    row = dict(parent_us=[round(x, 2) for x in p1], parent_again_us=[round(x, 2) for x in p2], parent_median_us=round(mp, 2),
               parent_vs_parent_max_us=round(pp, 2), builds={})
    for n, _ in builds:
        d = statistics.median(t[n]) - mp
        row["builds"][n] = dict(us=[round(x, 2) for x in t[n]], median_us=round(statistics.median(t[n]), 2), minus_parent_us=round(d, 2),
                                percent=round(100 * d / mp, 2), verdict="holds" if abs(d) <= pp else ("faster" if d < 0 else "SLOWER"))
    return row


def timing_line(kernel, row):
    line = f"{kernel:<34} parent {row['parent_median_us']:9.2f} us (pp {row['parent_vs_parent_max_us']:5.2f})"
    for n, b in row["builds"].items():
        line += f" | {n} {b['minus_parent_us']:+7.2f} us ({b['percent']:+.2f} %) {b['verdict']}"
    return line


def write_timing(path, rows, variants, rounds, reps, warm):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), rounds=rounds, reps=reps, warmup=warm, dropped_warmup_rounds=1,
                       variants=[n for n, _ in variants], cases=rows), f, indent=1)


def timing_args(argv):
    """[out.json] [name=variant.so ...] after --time -> (path or None, [(name, library)])"""
    rest = argv[argv.index("--time") + 1:]
    return next((a for a in rest if "=" not in a), None), [(a.split("=", 1)[0], load(a.split("=", 1)[1])) for a in rest if "=" in a]
