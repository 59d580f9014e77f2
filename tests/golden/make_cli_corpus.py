#!/usr/bin/env python3
"""Generates tests/golden/cli_corpus.json: what the analysis programs of 2022a-genome-dynamics_amd/host answer to a corpus of
command lines -- exit status, stdout and stderr of each.  The corpus is the expansion of one table per program (its options
with a value each accepts and the values its converters reject, its positionals, the options of its siblings) by the fixed
rules of expand() below.  tests/test_cli_corpus.py replays it, so the command lines of the programs stay what they were
when the corpus was recorded; a new option extends the program's table and the corpus is recorded again.

Every line but the empty one carries --dry-run, and no file named exists: no line reaches a device or writes a file, and no
recorded text holds a path of the recording machine (the programs run in an empty temporary directory).
Run:  python tests/golden/make_cli_corpus.py <directory of the built programs>"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))

LIST = ["x", "1,x", "1x", "0", "2,2", "1,", "4294967296"]          # parse_list: empty, no number, garbage, range, duplicate
COUNT = ["7x", "0", "268435457", "99999999999999999999"]            # 1 to 2^28
BOX = ["4,4", "4,4,4,4", "4,x,4", "0,4,4", "inf,4,4"]
NAME = ("fine", ["a/b"])
TRAJ = dict(positionals=["out.h5", "traj.h5"])
FLOW = {"--name": ("run1", []), "--smoothing": ("3", ["3.5", "-1"]), "--velocity-delay": ("2", ["x"]), "--scan-radius": ("1.5", ["1.5x"]), "--jobs": ("4", ["x"])}
RANGE = ["1", "1,2,3", "x,1", "1,x", ","]
BINSIZE = ("50000", ["x", "0", "-5", "1.5"])

# program (and command word) -> options: key -> (a value it accepts, values it rejects); flags besides --dry-run; required: the
# options a valid line needs; positionals: a valid list; limited: one more is an error; alias: short key -> the long key it
# stands for; foreign: options of sibling programs; extra: lines no rule makes
PROGRAMS = {
    "gd_msd": dict(TRAJ, options={"--name": NAME, "--lags": ("1,5,2", LIST), "--log-lags": ("7", COUNT), "--seps": ("3,4", ["2,2"]),
                                 "--log-seps": ("5", ["0"]), "--groups": ("chains", ["colour"])},
                   foreign=[["--smoothing", "3"], ["--bin-width", "0.5"]]),
    "gd_dcorr": dict(TRAJ, options={"--name": NAME, "--lags": ("1,5,2", ["1,x"]), "--log-lags": ("7", ["0"]), "--groups": ("types", ["chains"]),
                                   "--bin-width": ("0.5", ["0.5x", "0", "inf", "nan"]), "--max-distance": ("3", ["x", "1e9"]),
                                   "--origin-stride": ("2", ["0", "x", "4294967296"]), "--box": ("4,4,4", BOX)},
                     flags=["--split-chains", "--per-origin"], required=["--bin-width", "--max-distance"],
                     foreign=[["--seps", "1,2"], ["--thresholds", "1"]],
                     extra=[["--dry-run", "--bin-width", "0.5"], ["--bin-width", "0.5", "--max-distance", "3"]]),      # bins before positionals
    "gd_distance_map": dict(TRAJ, options={"--name": NAME, "--rebin-rate": ("4", ["0", "x", "268435457"]), "--chains": ("chr1,chr2", ["a,,b", "a,a"]),
                                          "--thresholds": ("1.5,2", ["x", "0", "inf", "1,,2", "1,2,3,4,5"]),
                                          "--frames": ("2:5", ["2", "x:5", "-1:5", "2:0", "4294967296:1", "2:5:1"]), "--box": ("4,4,4", BOX)},
                            flags=["--by-chain"], foreign=[["--lags", "1,2"], ["--groups", "all"]],
                            extra=[["--by-chain", "--rebin-rate", "4"], ["--dry-run", "--by-chain", "--rebin-rate=1"],      # the conflict before positionals
                                   ["--dry-run", "--by-chain", "--chains", "chr1", "out.h5", "traj.h5"]]),
    "gd_particle_flow": dict(TRAJ, options=FLOW, required=["--scan-radius"], foreign=[["--grid-interval", "1"], ["--x-range", "0,1"], ["--lags", "1"]]),
    "gd_grid_flow": dict(TRAJ, options=dict(FLOW, **{"--grid-interval": ("0.5", ["x", "0", "-1"]), "--x-range": ("-1,1", RANGE),
                                                    "--y-range": ("-2,2", ["x"]), "--z-range": ("0,0.5", ["1"])}),
                         required=["--scan-radius", "--grid-interval", "--x-range", "--y-range", "--z-range"], foreign=[["--lags", "1"]],
                         extra=[["--dry-run", "--scan-radius", "1"], ["--dry-run", "--scan-radius", "1", "--grid-interval", "1", "--x-range", "0,1"]]),
    "gd_rdf_analysis": dict(options={"--type": ("B", []), "--steps": ("10:20", ["x", "10:", "10:x", "10x", ":5", "99999999999999999999"]),
                                     "--bin-width": ("0.05", ["x", "1e999", "0.05x"]), "--max-distance": ("2", ["x"])},
                            flags=["-h", "--help"], positionals=["traj.h5"], limited=True, foreign=[["--name", "a"], ["-z"], ["-z", "1"]],
                            extra=[["-h"], ["--help", "--bogus"], ["--bogus", "--help"], ["--steps", "x", "--bin-width", "y", "traj.h5"]]),
    "gd_rdf_analysis_hetero": dict(options={"--type": ("B", []), "--bin-width": ("0.05", ["x", "1e999"]), "--max-distance": ("2", ["x"])},
                                   flags=["-h", "--help"], positionals=["traj.h5"], limited=True, foreign=[["--steps", "1:2"], ["-z"]], extra=[["--help"]]),
    "gd_analyze_lamina distance": dict(TRAJ, options={}, foreign=[["--name", "n1"], ["--contact-distance", "0.3"]]),
    "gd_analyze_lamina contact": dict(options={"--name": ("n1", []), "--contact-distance": ("0.3", ["x", "0.3x"])}, required=["--contact-distance"],
                                      positionals=["out.h5"], limited=True, foreign=[["--lags", "1"]]),
    "gd_analyze_lamina": dict(options={}, positionals=[], foreign=[],      # the word itself
                              extra=[["orbit", "--dry-run", "out.h5"], ["--dry-run", "orbit"], ["--name", "n1", "contact", "--contact-distance", "0.3", "out.h5"],
                                     ["--contact-distance", "0.3", "contact", "out.h5"], ["--contact-distance=0.3", "--dry-run", "contact", "out.h5"],
                                     ["distance", "contact", "--name", "n1", "--dry-run", "out.h5", "traj.h5"]]),
    "gd_contact_map": dict(options={"--after": ("100", ["x", "1.5", "99999999999999999999"]), "--before": ("900", ["x"]), "--chroms": ("chr1,chr2", [])},
                           required=["--chroms"], positionals=["jobdir"], limited=True, foreign=[["--frame-range", "1:2"], ["-o", "out.h5"], ["--output", "out.h5"]]),
    "gd_nad_profile": dict(options={"--after": ("100", ["x"]), "--before": ("900", ["1.5"]), "--chroms": ("chr1", [])},
                           required=["--chroms"], positionals=["jobdir"], limited=True, foreign=[["--rebin-rate", "2"], ["-o"]]),
    "gd_gw_contact_matrix": dict(options={"--frame-range": ("2:8", ["x", "2:x", "1:2:3", ":", "2:"]), "--rebin-rate": ("4", ["0", "x", "-1"]),
                                          "--output": ("out.h5", []), "-o": ("out.h5", [])},
                                 alias={"-o": "--output"}, required=["--output"], positionals=["a.h5", "b.h5"], foreign=[["--chroms", "chr1"], ["-z"], ["-z", "1"]],
                                 extra=[["--dry-run", "--frame-range", "3", "-o", "out.h5", "a.h5"], ["--dry-run", "--frame-range=-4:-1", "--output=out.h5", "a.h5"]]),
    "gd_power_law": dict(options={}, positionals=["a.h5", "b.h5"], foreign=[["--chroms", "x"], ["-o", "out"]]),
    "gd_compute_interactions": dict(options={"-b": BINSIZE, "-w": ("6", ["1", "x", "100000"]), "-o": ("out.tsv", [])}, required=["-b"],
                                    positionals=["in.mcool"], limited=True, foreign=[["-k", "3"], ["--binsize", "1000"], ["-z"], ["-z1"]]),
    "gd_compute_local_alpha": dict(options={"-w": ("10", ["0", "x", "4096"]), "-b": BINSIZE, "-o": ("out.tsv", [])},
                                   positionals=["in.mcool"], limited=True, foreign=[["-n", "KR"], ["--normalize", "KR"], ["-z"]]),
    "gd_hic_power_law": dict(options={"--binsize": BINSIZE, "--normalize": ("KR", [])}, positionals=["in.mcool"], limited=True,
                             foreign=[["-b", "1000"], ["-b1000"], ["-o", "x"]]),
    "gd_downsample": dict(options={"--rate": ("3", ["0", "x"]), "--window": ("5", ["-1", "x"]), "-o": ("out.tsv", [])},
                          positionals=["in.tsv"], limited=True, foreign=[["-w", "3"], ["-b5"]]),
    "gd_hic_compartments": dict(options={"-b": BINSIZE, "-n": ("KR", []), "-k": ("2", ["0", "x", "99"]), "--exclude": ("X,Y", []), "--chroms": ("1,2", [])},
                                positionals=["in.cool"], limited=True, foreign=[["-w", "3"], ["-o", "x"], ["--binsize", "5"]]),
}


def expand(table):
    """The command lines of one program's table, in a fixed order and without repeats."""
    options, flags, alias = table["options"], table.get("flags", []), table.get("alias", {})
    required, positionals = table.get("required", []), table["positionals"]

    def line(middle=(), drop=(), pos=positionals):      # --dry-run, the required options but `drop`, `middle`, the positionals
        head = [t for k in required if k not in drop for t in (k, options[k][0])]
        return ["--dry-run"] + head + list(middle) + list(pos)

    out = [[], ["--dry-run"], line(), line([t for k in options if k not in alias for t in (k, options[k][0])] + [f for f in flags if f.startswith("--") and f != "--help"], drop=required)]
    for k, (good, bad) in options.items():
        drop = [k, alias.get(k, k)]
        forms = [[k, good], [k + "=" + good]] if k.startswith("--") else [[k, good], [k + good]]
        rejected = [[k + "="] if k.startswith("--") else [k, ""]] + [[k, v] for v in bad]      # the empty value first
        out += [line(m, drop) for m in forms + rejected] + [line(drop=drop) + [k]]      # last: the option as the last token
    some_long = next((k for k in options if k.startswith("--")), "--dry-run")
    unknown = [["--bogus", "1"], ["--dry-run=1"], [some_long[:-1] + "=1"]]      # the last: a prefix of a key is no key
    if any(not k.startswith("--") for k in options):
        unknown += [["-z"], ["-z", "1"], ["-z1"]]
    out += [line(m) for m in unknown + table["foreign"]] + [line() + ["--bogus"]]
    out += [line(drop=[k]) for k in required]
    out += [line(pos=positionals[:n]) for n in range(len(positionals))]
    if table.get("limited"):
        out.append(line() + ["surplus"])
    out += [line(pos=[t] + positionals) for t in ("--", "-5")]      # tokens at the edge of the option syntax
    out += table.get("extra", [])
    seen = []
    for args in out:
        if args not in seen:
            seen.append(args)
    return seen


def corpus():
    for name, table in PROGRAMS.items():
        program, _, word = name.partition(" ")
        for args in expand(table):
            yield program, ([word] if word else []) + args


def run(host, program, args, cwd):
    r = subprocess.run([os.path.join(host, program), *args], capture_output=True, text=True, cwd=cwd, timeout=60)
    return {"program": program, "args": args, "status": r.returncode, "stdout": r.stdout, "stderr": r.stderr}


def main():
    host = os.path.abspath(sys.argv[1])
    with tempfile.TemporaryDirectory() as cwd:
        entries = [run(host, program, args, cwd) for program, args in corpus()]
        assert os.listdir(cwd) == [], "a command line of the corpus wrote a file"
    path = os.path.join(HERE, "cli_corpus.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e) for e in entries) + "\n]\n")
    print(f"{len(entries)} entries, {os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
