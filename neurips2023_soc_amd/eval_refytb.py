"""Per-expression J&F of a Ref-YouTube-VOS style results directory on the MI355X (refytb_eval, K27b):

    python -m neurips2023_soc_amd.eval_refytb --results_path RUNS --root DATA [--split valid] [--no-void] [--bound-th 0.008]

RUNS holds <video>/<exp_id>/<frame>.png as infer_refytb writes them; DATA holds <split>/Annotations and a
meta_expressions.json whose expressions carry obj_id.  Prints the global row and the per-expression table and writes
global_results-<split>.csv and per-expression_results-<split>.csv into RUNS.
"""
from __future__ import annotations

import argparse
import sys
from time import time

from . import refytb_eval


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--results_path", type=str, required=True,
                    help="Path to the folder containing the <video>/<exp_id> folders of mask PNGs")
    ap.add_argument("--root", type=str, required=True,
                    help="Dataset root with <split>/Annotations and meta_expressions/<split>/meta_expressions.json (with obj_id)")
    ap.add_argument("--split", type=str, default="valid", help="Split to evaluate the results on")
    ap.add_argument("--no-void", action="store_true", help="treat label 255 of the ground truth as background, not as void")
    ap.add_argument("--bound-th", type=float, default=0.008,
                    help="boundary tolerance: a fraction of the image diagonal, or a whole number of pixels when >= 1")
    a = ap.parse_args(argv)
    if not a.bound_th > 0 or (a.bound_th >= 1 and a.bound_th != int(a.bound_th)):
        ap.error("--bound-th is a positive fraction of the image diagonal, or a whole number of pixels when >= 1")
    return a


def main(argv=None) -> int:
    time_start = time()
    a = parse_args(argv)
    print(f"Evaluating expressions of the {a.split} split...")
    result = refytb_eval.evaluate(a.results_path, a.root, a.split, bound_th=a.bound_th, use_void=not a.no_void)
    path_g, path_e = refytb_eval.write_csvs(result, a.results_path, a.split)
    print(f"Global results saved in {path_g}")
    print(f"Per-expression results saved in {path_e}")
    print(refytb_eval.format_tables(result, a.split))
    sys.stdout.write("\nTotal time:" + str(time() - time_start) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
