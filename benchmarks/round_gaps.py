"""Per-round GPU busy/idle split from a rocprofv3 rocpd .db.

A boosting round starts at its ``grad_fused_kernel`` dispatch. For the
last N complete rounds of the trace this prints, per round (mean): the
span, the union of kernel (and, when traced, memory-copy) busy time, the
idle remainder, and the number of launches, blit copies and fills.

Usage: python benchmarks/round_gaps.py <results.db> [n_rounds=30]
"""

import sqlite3
import sys


def _table(cur, prefix):
    rows = cur.execute(
        "SELECT name FROM sqlite_master WHERE type='table' AND name LIKE ?",
        (prefix + "%",),
    ).fetchall()
    return rows[0][0] if rows else None


def round_gaps(dbf, n_rounds=30):
    cur = sqlite3.connect(dbf).cursor()
    kd = _table(cur, "rocpd_kernel_dispatch")
    ks = _table(cur, "rocpd_info_kernel_symbol")
    disp = cur.execute(
        f"SELECT kd.start, kd.end, ks.display_name FROM {kd} kd "
        f"JOIN {ks} ks ON kd.kernel_id = ks.id ORDER BY kd.start"
    ).fetchall()
    copies = []
    mc = _table(cur, "rocpd_memory_copy")
    if mc:
        copies = cur.execute(
            f"SELECT start, end FROM {mc} ORDER BY start").fetchall()
    marks = [s for s, _, name in disp if "grad_fused_kernel" in str(name)]
    if len(marks) < 2:
        raise SystemExit("fewer than two rounds in the trace")
    marks = marks[-(n_rounds + 1):]
    t0, t1 = marks[0], marks[-1]
    n = len(marks) - 1
    inside = [(s, e, str(nm)) for s, e, nm in disp if t0 <= s < t1]
    cin = [(s, e) for s, e in copies if t0 <= s < t1]
    iv = sorted([(s, e) for s, e, _ in inside] + cin)
    busy, cur_s, cur_e = 0, None, None
    for s, e in iv:
        if cur_e is None or s > cur_e:
            if cur_e is not None:
                busy += cur_e - cur_s
            cur_s, cur_e = s, e
        else:
            cur_e = max(cur_e, e)
    if cur_e is not None:
        busy += cur_e - cur_s
    span = t1 - t0
    ksum = sum(e - s for s, e, _ in inside)
    blit = [x for x in inside if "copyBuffer" in x[2]]
    fills = [x for x in inside
             if "FillFunctor" in x[2] or "fillBuffer" in x[2]]
    small = [x for x in inside if x[1] - x[0] < 15000]
    print(f"rounds {n}")
    print(f"span/round            {span / n / 1e6:.3f} ms")
    print(f"busy (union)/round    {busy / n / 1e6:.3f} ms")
    print(f"idle/round            {(span - busy) / n / 1e6:.3f} ms")
    print(f"kernel time sum/round {ksum / n / 1e6:.3f} ms")
    print(f"launches/round        {len(inside) / n:.1f}")
    print(f"blit copies/round     {len(blit) / n:.1f} "
          f"({sum(e - s for s, e, _ in blit) / n / 1e6:.3f} ms)")
    print(f"fills/round           {len(fills) / n:.1f} "
          f"({sum(e - s for s, e, _ in fills) / n / 1e6:.3f} ms)")
    print(f"kernels < 15 us/round {len(small) / n:.1f} "
          f"({sum(e - s for s, e, _ in small) / n / 1e6:.3f} ms)")
    if mc:
        print(f"traced memcpy/round   {len(cin) / n:.1f} "
              f"({sum(e - s for s, e in cin) / n / 1e6:.3f} ms)")
    agg = {}
    for s, e, nm in inside:
        key = nm.split("(")[0][:60]
        a = agg.setdefault(key, [0, 0])
        a[0] += 1
        a[1] += e - s
    print("per round: calls, ms, kernel")
    for key, (c, t) in sorted(agg.items(), key=lambda kv: -kv[1][1])[:24]:
        print(f"  {c / n:6.1f} {t / n / 1e6:7.3f}  {key}")


if __name__ == "__main__":
    round_gaps(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 30)
