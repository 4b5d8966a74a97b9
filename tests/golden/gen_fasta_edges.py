#!/usr/bin/env python3
"""Generate tests/golden/fasta_edges.json by running the REFERENCE's parser.

Like gen_golden.py this runs only where the reference (kmermaid 1.0.0) is
present; its directory is the one argument.  Every small
case of tests/fasta_cases.py that the reference can parse is written to a
scratch file and read back with its own SmartFastaParser (kmermaid/parsers.py,
loaded by path: the module imports the standard library only).  The fixture
holds, per case, the sha256 of the titles and cleaned sequences it yielded
(fasta_cases.digest), and the names of the cases left out with the reason.

Usage:  python tests/golden/gen_fasta_edges.py REFERENCE_DIR
"""

from __future__ import annotations

import importlib.util
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True
import fasta_cases as fc  # noqa: E402

LOOPS = "a record after the first has no sequence line: the reference's parser yields it forever"


def main() -> None:
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    src = os.path.join(sys.argv[1], "kmermaid", "parsers.py")
    if not os.path.isfile(src):
        sys.exit("no kmermaid/parsers.py under %s" % sys.argv[1])
    spec = importlib.util.spec_from_file_location("ref_parsers", src)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    digests, left_out = {}, {}
    with tempfile.TemporaryDirectory(prefix="kman_edges_") as d:
        path = os.path.join(d, "case.fa")
        for name, (text, _) in fc.small_cases().items():
            if fc.reference_loops(text):
                left_out[name] = LOOPS
                continue
            with open(path, "wb") as fh:
                fh.write(text)
            recs = [(t.encode("latin-1"), s.encode("latin-1")) for t, s in mod.SmartFastaParser.parse_file(path)]
            digests[name] = fc.digest(recs)
    with open(os.path.join(HERE, "fasta_edges.json"), "w") as fh:
        json.dump({"digests": digests, "left_out": left_out,
                   "generated_with": "kmermaid 1.0.0 SmartFastaParser.parse_file, python " + sys.version.split()[0]},
                  fh, indent=1, sort_keys=True)
    print("%d cases pinned, %d left out" % (len(digests), len(left_out)))


if __name__ == "__main__":
    main()
