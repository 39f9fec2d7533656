"""Child of tests/test_decoder_gpu.py's kernel-trace test, run under rocprofv3 in a process of its own: the cases of tests/decoder_cases.py and one launch of
every small kernel of libfeather_decoder.so (the results are held to the restatement by the parametrised tests, not here).  It prints the routes fhip_decoder_route named, in launch order, for
the parent to hold against the trace."""
import numpy as np
import torch

import decoder_cases as C
import side_contract
from feathercnn_amd import decoder as D


def main():
    lib = side_contract.library("decoder")
    seen = []
    for case in C.CASES:
        _, route, splits = C.run(lib, case)
        seen += [route] + [D.decoder_route(D.COMBINE)] * (splits > 1)
    x = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (1, 2, 3, 6)).astype(np.float32)).cuda()
    for t, vec in ((x[..., :4].contiguous(), 1), (x, 0)):  # d 4 in 16-byte units, d 6 in floats
        D.kv_concat(t, t)
        seen.append(D.decoder_route(D.KV_CONCAT, vec))
    for l in (6, 300):
        D.rms_norm(torch.ones((2, l), device="cuda"))
        seen.append(D.decoder_route(D.RMS_NORM, l))
    for interleaved in (0, 1):
        D.rotary(x, x[0, 0, :, :3].contiguous(), x[0, 1, :, :3].contiguous(), bool(interleaved))
        seen.append(D.decoder_route(D.ROTARY, interleaved))
    D.embed(torch.zeros(4, dtype=torch.int32, device="cuda"), x.reshape(6, 6))
    seen.append(D.decoder_route(D.EMBED))
    torch.cuda.synchronize()
    for name in seen:
        print("route " + name)
    print(f"{len(seen)} launches of {len(set(seen))} routes")
    print("child ok")


if __name__ == "__main__":
    main()
