"""Generates tests/golden/net_plan_snapshot.json on the MI355X: what the introspection API of feather::Net reports for every row of
tests/plan_snapshot_cases.py, from the build of the tree this script stands in.  Run:  python tests/golden/make_net_plan_snapshot.py [OUT]

The committed file comes from the commit before the convolution layer's state was regrouped (net_conv.h); the test holds every later
tree to it, value for value.  Regenerate it only with a change that means to alter what is fused or planned."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import plan_snapshot_cases as PS  # noqa: E402


def dumps(doc):
    """One line per layer / convolution row: readable diffs at a few tens of KB."""
    def flat(v):
        return json.dumps(v, separators=(",", ":"))

    def block(v):
        if isinstance(v, dict):
            return "{" + ",\n".join(f"{json.dumps(k)}:{flat(x)}" for k, x in v.items()) + "}"
        return "[" + ",\n".join(flat(x) for x in v) + "]"

    lines = ['{"conv_param_fields":' + flat(doc["conv_param_fields"]) + ',\n"cases":{']
    cases = []
    for rid, steps in doc["cases"].items():
        cases.append(json.dumps(rid) + ":[\n" + ",\n".join(
            "{" + ",\n".join(f"{json.dumps(k)}:{block(v) if k in ('layers', 'conv_params', 'fused_pointwise') else flat(v)}" for k, v in st.items()) + "}"
            for st in steps) + "]")
    return lines[0] + "\n" + ",\n".join(cases) + "}}\n"


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "net_plan_snapshot.json")
    doc = {"conv_param_fields": PS.conv_param_fields(), "cases": {row[0]: PS.run(row) for row in PS.table()}}
    text = dumps(doc)
    assert json.loads(text) == doc
    with open(path, "w") as f:
        f.write(text)
    print("wrote", path, len(text), "bytes,", len(doc["cases"]), "cases")


if __name__ == "__main__":
    main()
