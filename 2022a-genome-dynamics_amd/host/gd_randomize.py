#!/usr/bin/env python3
"""gd_randomize -- randomised controls of a genome bead table: the A/B classification shuffled, everything else kept.

The reference's `randomize [--seed S] [--preserve-structure | --completely-random] [-o OUT] <genome>`
(2-signal/src/randomize/__main__.py:16-23, randomize.py:11-69), host only: the rows' A and B values are permuted among the rows
(default), among the rows that carry no structural tag -- cen, anor, bnor -- (--preserve-structure), or replaced by a fair coin,
A = 0 / 1 and B = 1 - A (--completely-random, drawn after the permutation as in the reference); then the A / B / u letter of every
row's tags follows the sign of A - B.  The chain, start, end and tags columns stay on their rows, so a control has the beads, chains,
nucleolar ranges and bonds of its model and differs in the per-bead (a, b) factors alone: gd_prepare makes the model's and the
controls' trajectory files, and gd_interphase runs them as the replicas of one batch.

np.random.RandomState with the reference's draw order, and the reference's formatting of a row (a column that holds integers only is
written as integers, any other numeric column as the shortest round-trip decimals): the output is the reference's byte for byte
(tests/golden/randomize_*.tsv, recorded from the reference's module).  The seed in use goes to stderr, so that a run without --seed
can be repeated.
"""
import argparse
import csv
import sys

import numpy as np

STRUCTURAL_ELEMENTS = ["cen", "anor", "bnor"]


def _column(cells):
    """A column as the table reader of the reference types it: int64 if every cell is an integer, else float64, else text"""
    for dtype in (np.int64, np.float64):
        try:
            return np.array([dtype(c) for c in cells], dtype=dtype)
        except ValueError:
            pass
    return list(cells)


def read_table(filename):
    with open(filename, newline="") as fh:
        rows = list(csv.reader(fh, delimiter="\t"))
    header, rows = rows[0], [r for r in rows[1:] if r]
    for k, r in enumerate(rows):
        if len(r) != len(header):
            raise SystemExit(f"error: {filename}: row {k + 1} has {len(r)} columns, the header {len(header)}")
    for name in ("A", "B", "tags"):
        if name not in header:
            raise SystemExit(f"error: {filename}: no column '{name}'")
    return header, {name: _column([r[c] for r in rows]) for c, name in enumerate(header)}


def randomize(table, seed, preserve_structure=False, completely_random=False):
    """The reference's run() on the columns of `table` (in place)"""
    random = np.random.RandomState(seed=seed)
    A, B, tags = table["A"], table["B"], table["tags"]
    n = len(tags)
    if isinstance(A, list) or isinstance(B, list):
        raise SystemExit("error: the A and B columns must be numeric")
    order = np.arange(n)
    if preserve_structure:
        selector = np.array([not any(x in t for x in STRUCTURAL_ELEMENTS) for t in tags], dtype=bool)
        sub_order = order[selector]
        random.shuffle(sub_order)
        order[selector] = sub_order
    else:
        random.shuffle(order)
    A[:] = A[order]
    B[:] = B[order]
    if completely_random:
        A[:] = random.randint(2, size=n)
        B[:] = 1 - A
    for i in range(n):      # the A / B / u letter follows the factors
        delta_ab = A[i] - B[i]
        if delta_ab > 0:
            tags[i] = tags[i].replace("B", "A").replace("u", "A")
        elif delta_ab < 0:
            tags[i] = tags[i].replace("A", "B").replace("u", "B")
        else:
            tags[i] = tags[i].replace("A", "u").replace("B", "u")


def write_table(output, header, table):
    output.write("\t".join(header) + "\n")
    for i in range(len(table["tags"])):
        output.write("\t".join(str(table[name][i]) for name in header) + "\n")


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--seed", type=int, default=None)
    parser.add_argument("--preserve-structure", action="store_true", default=False)
    parser.add_argument("--completely-random", action="store_true", default=False)
    parser.add_argument("-o", dest="outfile", type=str, default=None)
    parser.add_argument("infile", type=str)
    args = parser.parse_args()
    if args.preserve_structure and args.completely_random:
        raise SystemExit("error: --preserve-structure and --completely-random options can not both be specified")
    seed = args.seed if args.seed is not None else int(np.random.randint(2 ** 31 - 1))
    print(f"[gd_randomize] seed {seed}", file=sys.stderr)
    header, table = read_table(args.infile)
    randomize(table, seed, args.preserve_structure, args.completely_random)
    if args.outfile is None:
        write_table(sys.stdout, header, table)
    else:
        with open(args.outfile, "w") as fh:
            write_table(fh, header, table)


if __name__ == "__main__":
    try:
        main()
    except BrokenPipeError:
        sys.exit(1)
