import os
import re

import numpy as np

import oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_golden.npz")
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "feathercnn_amd", "csrc")


def net_runtime_source():
    """The Net runtime as one text: feathercnn_amd/csrc/net.hip followed by every csrc/net_*.h it includes (directly or through
    another of them), each once, in include order.  A csrc/net_*.h that nothing includes is an error: the tests that read the
    runtime as text must see all of it."""
    seen, parts = [], []

    def visit(name):
        text = open(os.path.join(CSRC, name)).read()
        for inc in re.findall(r'^#include "(net_\w+\.h)"', text, re.M):
            if inc not in seen:
                seen.append(inc)
                visit(inc)
        parts.append(text)

    visit("net.hip")
    on_disk = {f for f in os.listdir(CSRC) if re.fullmatch(r"net_\w+\.h", f)}
    assert on_disk == set(seen), sorted(on_disk ^ set(seen))
    return parts[-1] + "".join(parts[:-1])


def net_layer_types():
    """(types create_layer accepts, types create_extended_layer accepts), read out of the two factories of net.hip."""
    src = net_runtime_source()
    out = []
    for fn in ("static Layer* create_layer(", "static Layer* create_extended_layer("):
        body = src[src.index(fn):]
        out.append(set(re.findall(r'type == "(\w+)"', body[:body.index("\n}\n")])))
    return out[0], out[1]


def golden_cases():
    """-> list of (name, Geom, batch, forced_algo, x, w, b, y_ref, selected_algo) from the committed reference fixtures."""
    z = np.load(GOLDEN)
    names = sorted({k.split("/")[0] for k in z.files})
    out = []
    for n in names:
        g15 = z[n + "/geom"]
        g = oracle.Geom(*[int(v) for v in g15[:15]])
        out.append((n, g, int(g15[15]), int(g15[16]), z[n + "/x"], z[n + "/w"], z[n + "/b"], z[n + "/y"], int(z[n + "/algo"][0])))
    return out
