"""DAVIS J&F of a results directory, the reference's eval_davis.py on the MI355X:

    python -m neurips2023_soc_amd.eval_davis --davis_path DAVIS --results_path RUNS/anno_0 [--set val] [--task unsupervised]

Flags and defaults are the reference's (eval_davis.py:15-23), without its author's absolute paths.  Writes
global_results-<set>.csv and per-sequence_results-<set>.csv into the results directory and prints both tables; when both
files exist already they are read back instead, as the reference does (:30-33).
"""
from __future__ import annotations

import argparse
import csv
import os
import sys
from time import time

from . import davis_eval


def _read_csv(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def main(argv=None) -> int:
    time_start = time()
    ap = argparse.ArgumentParser()
    ap.add_argument("--davis_path", type=str, required=True,
                    help="Path to the DAVIS folder containing the Annotations, ImageSets, Annotations_unsupervised folders")
    ap.add_argument("--set", type=str, default="val", help="Subset to evaluate the results")
    ap.add_argument("--task", type=str, default="unsupervised", choices=list(davis_eval.TASKS),
                    help="Task to evaluate the results")
    ap.add_argument("--results_path", type=str, required=True, help="Path to the folder containing the sequences folders")
    args, _ = ap.parse_known_args(argv)
    path_g, path_seq = davis_eval.csv_paths(args.results_path, args.set)
    if os.path.exists(path_g) and os.path.exists(path_seq):
        print("Using precomputed results...")
        row_g, rows_seq = _read_csv(path_g)[1], _read_csv(path_seq)[1:]
    else:
        print(f"Evaluating sequences for the {args.task} task...")
        result = davis_eval.evaluate(args.results_path, args.davis_path, args.task, args.set)
        davis_eval.write_csvs(result, args.results_path, args.set)
        print(f"Global results saved in {path_g}")
        print(f"Per-sequence results saved in {path_seq}")
        row_g, rows_seq = result.global_row(), result.per_sequence()
    print(davis_eval.format_tables(row_g, rows_seq, args.set))
    sys.stdout.write("\nTotal time:" + str(time() - time_start) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
