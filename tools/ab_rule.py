"""The keep rule on the rows of an alternating A/B (library, run, ms_per_step, ...):
every new run faster than every parent run, and the difference of the medians
at least three times the parent's own range in that session.
    python tools/ab_rule.py rows.txt [parent [new [label]]]
prints one summary line in the form of profiles/r12/guards/ab.txt."""
import statistics
import sys


def summary(rows, parent="parent", new="new", label=None):
    p = [float(r[2]) for r in rows if r[0] == parent]
    n = [float(r[2]) for r in rows if r[0] == new]
    mp, mn = statistics.median(p), statistics.median(n)
    rng = max(p) - min(p)
    every = max(n) < min(p)
    times = (mp - mn) / rng if rng > 0 else float("inf")
    return (f"## {label or new}: median {mp:.3f} -> {mn:.3f} ms ({mn - mp:+.3f} ms, {100 * (mn - mp) / mp:+.1f} %); "
            f"parent {min(p):.3f}-{max(p):.3f} (range {rng:.3f}), new {min(n):.3f}-{max(n):.3f}; "
            f"every new run faster than every parent run: {'yes' if every else 'NO'}; "
            f"difference of medians = {times:.1f} x the parent's range")


if __name__ == "__main__":
    rows = [l.split() for l in open(sys.argv[1]) if len(l.split()) >= 3 and not l.startswith("#")]
    print(summary(rows, *(sys.argv[2:5])))
