"""Child process of tests/test_shuffle_gpu.py's kernel-trace test: one Forward of Concat -> ShuffleChannel(2) -> Slice(2) between two Input
blobs at the fusion level given on the command line, bracketed by two fhip_relu launches so that the trace can be cut at them (the feeds
and the extraction copy too)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

PARAM = (b"7767517\n5 6\nInput a 0 1 a 0=14 1=14 2=116\nInput b 0 1 b 0=14 1=14 2=116\nConcat cat 2 1 a b cat 0=0\n"
         b"ShuffleChannel sh 1 1 cat sh 0=2\nSlice sl 1 2 sh keep work -23300=2,-233,-233\n")


def main():
    import shuffle_ref as R
    from feathercnn_amd.net import Net
    level = int(sys.argv[1])
    rng = np.random.default_rng(1)
    a, b = (rng.normal(0, 1, (4, 116, 14, 14)).astype(np.float32) for _ in range(2))
    net = Net(fusion=level)
    net.LoadParam(PARAM)
    net.LoadWeights(b"")
    net.FeedInput("a", a)
    net.FeedInput("b", b)
    net.Forward()  # the first Forward reshapes and builds the table; the traced one only launches
    import ktrace
    ktrace.marker()
    net.Forward()
    ktrace.marker()
    keep, work = net.Extract("keep"), net.Extract("work")
    net.close()
    want = R.channel_slice(R.channel_shuffle(np.concatenate([a, b], 1), 2), [-233, -233])
    assert np.array_equal(keep, want[0]) and np.array_equal(work, want[1])
    print("child ok")


if __name__ == "__main__":
    main()
