"""Which layer types make a net need a weight file: for every type the two factories of the Net runtime accept, a net of `Input` plus
that one layer on a 1x4x6x6 blob is fed and run WITHOUT LoadWeights.

  * a type whose LoadWeights reads the .bin -- Convolution, ConvolutionDepthWise, Deconvolution, DeconvolutionDepthWise, InnerProduct,
    InstanceNorm (also with affine=0), PReLU, BatchNorm, Scale -- is refused with NET_E_IO (-1) and "weights have not been loaded";
  * every other type, a Scale that takes its scale from a second bottom (0=-233) among them, runs.

WEIGHTS below is the claim, a literal table; test_every_type_is_classified holds its keys against the factories, so that a new layer type
fails here until it is classified.  The layer lines take their parameters from the base models of tests/loader_cases.py where a model
holds the type, cut down to four channels."""
import pytest

import helpers

pytestmark = pytest.mark.gpu

# the inputs a case may name as bottoms: blob -> shape
INPUTS = {"data": (1, 4, 6, 6), "other": (1, 4, 6, 6), "gate": (1, 4, 1, 1)}

# case -> (needs a weight file, bottoms, number of tops, params); the type is the case's name up to ':'
WEIGHTS = {
    "Input": (False, (), 1, ""),
    "Convolution": (True, ("data",), 1, "0=4 1=3 4=1 5=1 6=144"),
    "ConvolutionDepthWise": (True, ("data",), 1, "0=4 1=3 4=1 5=1 6=36 7=4"),
    "Deconvolution": (True, ("data",), 1, "0=4 1=2 3=2 5=1 6=64"),
    "DeconvolutionDepthWise": (True, ("data",), 1, "0=4 1=2 3=2 5=1 6=16 7=4"),
    "InnerProduct": (True, ("data",), 1, "0=3 1=1 2=432"),
    "InstanceNorm": (True, ("data",), 1, "0=4 1=0.001 2=1"),
    "InstanceNorm:affine0": (True, ("data",), 1, "0=4 1=0.001 2=0"),
    "PReLU": (True, ("data",), 1, "0=4"),
    "BatchNorm": (True, ("data",), 1, "0=4 1=0.001"),
    "Scale": (True, ("data",), 1, "0=4 1=1"),
    "Scale:gated": (False, ("data", "gate"), 1, "0=-233"),
    "ReLU": (False, ("data",), 1, ""),
    "ReLU:leaky": (False, ("data",), 1, "0=0.1"),
    "Sigmoid": (False, ("data",), 1, ""),
    "TanH": (False, ("data",), 1, ""),
    "Clip": (False, ("data",), 1, "0=-1.0 1=1.0"),
    "Pooling": (False, ("data",), 1, "0=0 1=2 2=2"),
    "Dropout": (False, ("data",), 1, ""),
    "Dropout:scaled": (False, ("data",), 1, "0=0.5"),
    "Softmax": (False, ("data",), 1, ""),
    "Split": (False, ("data",), 2, ""),
    "Eltwise": (False, ("data", "other"), 1, "0=1"),
    "Concat": (False, ("data", "other"), 1, "0=0"),
    "ShuffleChannel": (False, ("data",), 1, "0=2"),
    "Slice": (False, ("data",), 2, "-23300=2,1,-233"),
    "BinaryOp": (False, ("data", "gate"), 1, "0=2"),
    "Swish": (False, ("data",), 1, ""),
    "HardSigmoid": (False, ("data",), 1, "0=0.2 1=0.5"),
    "Interp": (False, ("data",), 1, "0=2 1=2.0 2=2.0"),
    "HardSwish": (False, ("data",), 1, "0=0.1666667 1=0.5"),
    "LRN": (False, ("data",), 1, "0=0 1=5 2=0.0001 3=0.75"),
}


def _param(case):
    _, bottoms, tops, pairs = WEIGHTS[case]
    type_ = case.split(":")[0]
    fed = list(INPUTS) + (["top0"] if type_ == "Input" else [])
    names = " ".join(f"top{j}" for j in range(tops))
    text = (f"7767517\n2 {len(INPUTS) + tops}\nInput in 0 {len(INPUTS)} {' '.join(INPUTS)}\n"
            f"{type_} layer {len(bottoms)} {tops} {' '.join(bottoms)} {names} {pairs}\n")
    return text.encode(), fed


def test_every_type_is_classified():
    plain, extended = helpers.net_layer_types()
    assert len(plain) >= 25 and extended >= {"Interp", "HardSwish", "LRN"} and not plain & extended
    assert {c.split(":")[0] for c in WEIGHTS} == plain | extended


@pytest.mark.parametrize("case", sorted(WEIGHTS))
def test_forward_without_a_weight_file(cuda, case):
    import numpy as np
    from feathercnn_amd.booster import FeatherHipError
    from feathercnn_amd.net import Net
    param, fed = _param(case)
    net = Net()
    net.SetDilated(True)
    net.SetExtendedLayers(True)
    net.LoadParam(param)
    rng = np.random.default_rng(3)
    for name in fed:
        net.FeedInput(name, rng.uniform(-1, 1, INPUTS.get(name, INPUTS["data"])).astype(np.float32))
    try:
        net.Forward()
        said = None
    except FeatherHipError as e:
        said = str(e)
    finally:
        net.synchronize()
    net.close()
    if WEIGHTS[case][0]:
        assert said is not None and "code -1:" in said and "weights have not been loaded" in said, said
    else:
        assert said is None, said
