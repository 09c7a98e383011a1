"""Record which names the reference's entry scripts import from the `open_musiclm` package (build container only):

    python oracle/make_script_imports.py

  tests/golden/reference_script_imports.json   {script: {module: [names]}} for every `from open_musiclm.<module> import ...`
                                               of scripts/train_*.py and scripts/preprocess_data.py, read from their syntax
                                               trees (nothing is executed): the drop-in surface the alias package
                                               (open_musiclm/__init__.py) must provide, pinned for machines without the reference.
"""
from __future__ import annotations

import ast
import json
import os
import sys

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle.make_golden import OUT, REF  # noqa: E402

SCRIPTS = ("train_semantic_stage", "train_coarse_stage", "train_fine_stage", "train_clap_rvq", "train_hubert_kmeans", "preprocess_data")


def package_imports(path):
    out = {}
    for node in ast.walk(ast.parse(open(path).read(), path)):
        if isinstance(node, ast.ImportFrom) and node.level == 0 and node.module and node.module.split(".")[0] == "open_musiclm":
            out.setdefault(node.module, []).extend(a.name for a in node.names)
        elif isinstance(node, ast.Import):
            assert not any(a.name.split(".")[0] == "open_musiclm" for a in node.names), (path, "plain import: extend the fixture format")
    return {m: sorted(set(n)) for m, n in sorted(out.items())}


def main():
    data = {s: package_imports(os.path.join(REF, "scripts", f"{s}.py")) for s in SCRIPTS}
    assert all(data.values()), data
    with open(os.path.join(OUT, "reference_script_imports.json"), "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
