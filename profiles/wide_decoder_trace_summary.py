"""Per-launch-shape kernel times from a rocprofv3 --kernel-trace CSV of profiles/wide_decoder.py: the two k_decw_out
variants (log-probs: grid G x tiles, tokens only: 1 x tiles) have different grids, which the --stats table averages
together.  Writes one row per (kernel, grid): calls, median / min / max duration in microseconds.

    python profiles/wide_decoder_trace_summary.py <..._kernel_trace.csv> profiles/wide_decoder_rocprof_kernels.csv
"""
import collections
import csv
import statistics
import sys

KERNELS = ('k_decw_stats', 'k_decw_out', 'k_dec(', 'k_logsoftmax', 'k_sep<0, 1, 0, false, 32>')


def main(src, dst):
    d = collections.defaultdict(list)
    with open(src) as f:
        for r in csv.DictReader(f):
            name = r['Kernel_Name']
            k = next((k for k in KERNELS if k in name), None)
            if k:
                grid = f"{r['Grid_Size_X']}x{r['Grid_Size_Y']}x{r['Grid_Size_Z']}"
                d[(k.rstrip('('), grid)].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    with open(dst, 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['kernel', 'grid_threads', 'calls', 'median_us', 'min_us', 'max_us'])
        for (k, grid), v in sorted(d.items()):
            w.writerow([k, grid, len(v), round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)])


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
