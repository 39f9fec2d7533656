"""Child of tests/test_q8_gpu.py's kernel-trace test, run under rocprofv3 in a process of its own: the sweep of tests/q8_sweep.py (every
route of every form of every case of tests/q8_cases.py, compared with the restatement as it goes) and the four tensor calls."""
import numpy as np

import q8_ref as Q
import q8_sweep as SW
import side_contract


def main():
    import torch
    from feathercnn_amd import q8_max_pool, q8_pack, q8_relu, q8_unpack
    lib = side_contract.library("q8")
    seen = []

    def check(name, form, route, got, want):
        got = got[0] if form[1] else got
        assert np.array_equal(got, want), (name, form, route)
        seen.append(route)

    SW.sweep(lib, check)
    x = torch.from_numpy(np.random.default_rng(1).uniform(-3, 3, (2, 20, 6, 6)).astype(np.float32)).cuda()
    t = q8_max_pool(q8_relu(q8_pack(x, 40.0)), 20)
    y = q8_unpack(t, 20, 40.0)
    torch.cuda.synchronize()
    want = Q.dequantize(Q.pack(Q.max_pool(Q.relu(Q.unpack(Q.quantize(x.cpu().numpy(), 40.0), 20)))), 20, 40.0)
    assert np.array_equal(y.cpu().numpy(), want)
    print(f"{len(seen)} launches of {len(set(seen))} routes")
    print("child ok")


if __name__ == "__main__":
    main()
