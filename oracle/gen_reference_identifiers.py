#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- generate tests/golden/reference_ceed_identifiers.json.

The Ceed* / CEED_* identifiers the reference's C sources use (comments and string literals stripped), and those of them that
are the reference's OWN names (its CeedData struct family, functions it defines itself): two sorted lists of names, no program
text.  tests/test_boundary_compile.py checks that include/ceed.h declares every used name that is not the reference's own.

    python oracle/gen_reference_identifiers.py <reference tree>   # rewrites tests/golden/reference_ceed_identifiers.json
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOURCES = ["src/setuplibceed.c", "src/matops.c", "src/misc.c", "src/boundary.c", "src/cloptions.c", "src/setupdm.c", "elasticity.c", "elasticity.h"]
IDENT = r"\b(Ceed[A-Za-z0-9_]*|CEED_[A-Z0-9_]+)\b"


def identifiers(ref: str):
    own, used = set(), set()
    for src in SOURCES:
        txt = open(os.path.join(ref, src)).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        txt = re.sub(r"//[^\n]*", "", txt)
        txt = re.sub(r'"(?:\\.|[^"\\])*"', '""', txt)                       # string literals (option prefixes such as "CEED_MEM_")
        used |= set(re.findall(IDENT, txt))
        own |= set(re.findall(r"(?:struct|typedef struct)\s+(Ceed[A-Za-z0-9_]*)", txt))
        own |= set(re.findall(r"}\s*\*?\s*(Ceed[A-Za-z0-9_]*)\s*;", txt))
        own |= set(re.findall(r"typedef\s+struct\s+\w+\s*\*\s*(Ceed[A-Za-z0-9_]*)\s*;", txt))
        own |= set(re.findall(r"PetscErrorCode\s+(Ceed[A-Za-z0-9_]*)\s*\(", txt))       # functions the reference defines itself
    return {"sources": SOURCES, "used": sorted(used), "own": sorted(own & used)}


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    out = os.path.join(ROOT, "tests", "golden", "reference_ceed_identifiers.json")
    with open(out, "w") as f:
        json.dump(identifiers(sys.argv[1]), f, indent=1)
        f.write("\n")
    print("wrote", out)
