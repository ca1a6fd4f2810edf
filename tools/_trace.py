"""tools/_trace.py -- the rate tools' kernel trace: run the calling tool again as a fresh child under `rocprofv3 --kernel-trace --stats`
and read what it wrote.  No counters and no other tracing mode."""
import csv
import glob
import os
import subprocess
import sys
import tempfile


def kernel_rows(args, tag, timeout, with_stats=False):
    """[(kernel name, start ns, end ns)] sorted by start, of `<python> <the calling tool> *args`; with_stats: (rows, the rows of the
    profiler's kernel statistics as dicts, [] if it wrote none)"""
    tool = os.path.abspath(sys._getframe(1).f_globals["__file__"])
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", tag, "--", sys.executable, tool] + list(args)
        subprocess.run(cmd, check=True, timeout=timeout, stdout=subprocess.DEVNULL)
        traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        assert traces, "rocprofv3 wrote no kernel trace"
        with open(traces[0]) as fh:
            rows = sorted(((row["Kernel_Name"], int(row["Start_Timestamp"]), int(row["End_Timestamp"])) for row in csv.DictReader(fh)),
                          key=lambda r: r[1])
        stat_rows = []
        if with_stats and stats:
            with open(stats[0]) as fh:
                stat_rows = [{k: row[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs") if k in row} for row in csv.DictReader(fh)]
    return (rows, stat_rows) if with_stats else rows
