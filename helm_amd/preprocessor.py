"""The benchmark suite's `preprocessor` step (reference README.md:116-120,133-137): raw Yosys netlists, or with
--arithmetic behavioural arithmetic Verilog, to the dialect verilog_parser reads.  Thin binding of
helm_host_preprocess (helm_amd/csrc/host/preprocessor.cpp).

    python -m helm_amd.preprocessor --input raw.v --output processed.v [--arithmetic] [--fuse3]

--fuse3 (opt-in, gates mode only) runs the three-input fusion pass over the result (verilog_parser.fuse3): its output
uses the keywords maj / xor3 / xnor3, which the reference's parser does not know.
"""
import argparse
import sys

from . import _host as H


def preprocess(text, arithmetic=False):
    return H.out_text(H.host.helm_host_preprocess, text.encode(), int(bool(arithmetic)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--input", required=True)
    ap.add_argument("--output", required=True)
    ap.add_argument("--arithmetic", action="store_true")
    ap.add_argument("--fuse3", action="store_true", help="fuse xor pairs and full-adder carries into three-input gates")
    a = ap.parse_args(argv)
    if a.fuse3 and a.arithmetic:
        ap.error("--fuse3 works on gates-mode netlists, not with --arithmetic")
    with open(a.input) as f:
        text = f.read()
    text = preprocess(text, a.arithmetic)
    if a.fuse3:
        from .verilog_parser import fuse3
        text, stats = fuse3(text)
        print(f"fuse3: bootstraps {stats[0]} -> {stats[1]}, bootstrapped levels {stats[2]} -> {stats[3]}", file=sys.stderr)
    with open(a.output, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
