#!/usr/bin/env python3
"""Generates tests/golden/randomize_{genome,default,preserve,random}.tsv by IMPORTING the reference's own randomize module
(2-signal/src/randomize/randomize.py) in this container and recording its outputs for one small genome bead table in its three
modes.  Only the input and the outputs are stored; run here (the reference tree does not exist on the GPU box):
python tests/golden/make_randomize_fixtures.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference/2-signal/src/randomize")
import randomize  # noqa: E402

SEED = 20220101
MODES = {"default": {}, "preserve": {"preserve_structure": True}, "random": {"completely_random": True}}


def genome():
    """Three chains of 100 kb beads: runs of A / B / u with fractional factors among them, a centromere and a NOR per chain, extra tags"""
    rng = np.random.default_rng(7)
    kinds = [(1.0, 0.0, "A"), (0.0, 1.0, "B"), (0.5, 0.5, "u"), (0.7, 0.3, "A"), (0.25, 0.75, "B")]
    rows = []
    for chain, n in (("chr1", 18), ("chr2", 14), ("chrX", 9)):
        cen, nor = n // 2, n - 3
        for k in range(n):
            a, b, letter = kinds[int(rng.integers(len(kinds)))]
            tags = [letter]
            if k in (cen, cen + 1):
                tags.append("cen")
            if k == nor:
                tags.append("anor" if a >= b else "bnor")
            if rng.random() < 0.2:
                tags.append("L1")
            rows.append((chain, k * 100000, (k + 1) * 100000, a, b, ",".join(tags)))
    return rows


def main():
    infile = os.path.join(HERE, "randomize_genome.tsv")
    with open(infile, "w") as fh:
        fh.write("chain\tstart\tend\tA\tB\ttags\n")
        for r in genome():
            fh.write("\t".join(str(v) for v in r) + "\n")
    for name, mode in MODES.items():
        kw = dict(preserve_structure=False, completely_random=False)
        kw.update(mode)
        randomize.run(infile=infile, outfile=os.path.join(HERE, f"randomize_{name}.tsv"), seed=SEED, **kw)
    print("ok", {name: os.path.getsize(os.path.join(HERE, f"randomize_{name}.tsv")) for name in ["genome", *MODES]})


if __name__ == "__main__":
    main()
