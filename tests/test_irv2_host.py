"""Inception-ResNet-v2: host-side checks (no GPU): variable counts, map sizes, the slim name table, v1 plans unchanged."""
import hashlib
import json
import os

import pytest

from facenet_amd.engine import Network
from facenet_amd.engine_v2 import NetworkV2, build_network, map_sizes, network_class
from tests.irv2_oracle import param_names
from tests.plan_signature import signature

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "v1_plan_signature.json")


@pytest.mark.parametrize("E, counts", [(128, (54533728, 54472928)), (512, (55124704, 55063136))])
def test_variable_counts(E, counts):
    assert NetworkV2(E, allocate=False, device="cpu").count_variables() == counts


def test_variable_breakdown_E128():
    net = NetworkV2(128, allocate=False, device="cpu")
    Ls = list(net.layers.values())
    assert sum(L.cout_real * L.kh * L.kw * L.cin_real for L in Ls) == 54396768
    assert sum(L.cout_real for L in Ls if L.has_bias) == 45760
    assert sum(L.cout for L in Ls if L.has_bn) == 30400 == net.CB


def test_map_sizes():
    assert map_sizes(160) == (17, 8, 3)
    assert map_sizes(299) == (35, 17, 8)
    for size, (s5, s6, s7) in ((160, (17, 8, 3)), (299, (35, 17, 8))):
        net = NetworkV2(128, image_size=size, allocate=False, device="cpu")
        assert net.count_variables() == (54533728, 54472928)     # whole-map pool: the head does not depend on the size
    with pytest.raises(ValueError):
        NetworkV2(128, image_size=60, allocate=False, device="cpu")


def test_config_keys_and_momentum():
    net = NetworkV2(allocate=False, device="cpu", config={"repeat": [1, 2, 1], "keep_probability": 0.8, "weight_decay": 1e-3,
                                                          "mixed_5a": {"branch": [[32], [16, 24], [16, 24, 32], [16]]}})
    assert net.E == 512 and net.keep_probability == 0.8 and net.l2_weight == 5e-4
    assert net.layers["Mixed_5a/Branch_1/Conv2d_0b_5x5"].cout == 24
    assert "Repeat_1/block17_2/Conv2d_1x1" in net.layers and "Repeat_1/block17_3/Conv2d_1x1" not in net.layers
    assert net.bn_momentum == 0.995 and Network.bn_momentum == 0.99
    assert net.layers["Repeat/block35_1/Conv2d_1x1"].cout == 104      # up width = the trunk's (Mixed_5a concat)


EXAMPLES = [
    "InceptionResnetV2/Conv2d_1a_3x3/weights",
    "InceptionResnetV2/Conv2d_1a_3x3/BatchNorm/beta",
    "InceptionResnetV2/Conv2d_1a_3x3/BatchNorm/moving_mean",
    "InceptionResnetV2/Conv2d_1a_3x3/BatchNorm/moving_variance",
    "InceptionResnetV2/Mixed_5a/Branch_1/Conv2d_0b_5x5/weights",
    "InceptionResnetV2/Repeat/block35_1/Branch_2/Conv2d_0c_3x3/weights",
    "InceptionResnetV2/Repeat/block35_1/Conv2d_1x1/weights",
    "InceptionResnetV2/Repeat/block35_1/Conv2d_1x1/biases",
    "InceptionResnetV2/Repeat/block35_10/Conv2d_1x1/biases",
    "InceptionResnetV2/Repeat_1/block17_20/Branch_1/Conv2d_0c_7x1/weights",
    "InceptionResnetV2/Repeat_2/block8_9/Branch_1/Conv2d_0b_1x3/weights",
    "InceptionResnetV2/Block8/Branch_0/Conv2d_1x1/weights",
    "InceptionResnetV2/Block8/Conv2d_1x1/biases",
    "InceptionResnetV2/Bottleneck/weights",
    "InceptionResnetV2/Bottleneck/BatchNorm/beta",
]


def test_name_table_is_a_bijection():
    net = NetworkV2(128, nrof_classes=10, allocate=False, device="cpu")
    table = net.variable_table()
    names, keys = [k for k, _ in table], [i for _, i in table]
    assert len(set(names)) == len(names) and len(set(keys)) == len(keys)
    engine = []
    for L in net.layers.values():
        engine.append(L.name + "/kernel")
        if L.has_bias:
            engine.append(L.name + "/bias")
        if L.has_bn:
            engine += [f"{L.name}/bn/{v}" for v in ("beta", "moving_mean", "moving_variance")]
    assert sorted(keys) == sorted(engine)
    for ex in EXAMPLES:
        assert ex in names, ex
    assert "Logits/weights" in names and "Logits/biases" in names
    assert not any(n.startswith("InceptionResnetV2/Repeat/block35_0") for n in names)


def test_restatement_names_match_table():
    net = NetworkV2(128, allocate=False, device="cpu")
    assert param_names(128) == [i for _, i in net.variable_table()]


def test_module_selection():
    assert network_class(None) is Network
    assert network_class("facenet.models.inception_resnet_v1") is Network
    assert network_class("facenet.models.inception_resnet_v2") is NetworkV2
    assert network_class("facenet_amd.models.inception_resnet_v2") is NetworkV2
    with pytest.raises(ValueError):
        network_class("facenet.models.squeezenet")
    from facenet_amd.config import Config
    net = build_network(Config({"module": "facenet.models.inception_resnet_v2", "config": {"repeat": [1, 1, 1]}}), 128,
                        allocate=False, device="cpu")
    assert isinstance(net, NetworkV2) and net.E == 128 and net.cfg["repeat"] == [1, 1, 1]


def test_v2_plan_lowers_on_host():
    """A v2 training plan (with dropout) and an inference plan lower without a GPU; dropout only in training."""
    net = NetworkV2(128, allocate=False, device="cpu", config={"repeat": [1, 1, 1]})
    tr = signature(net, 6, True)
    names = [op[0] for op in tr]
    assert "dropout_fwd" in names and "dropout_bwd" in names
    assert "avgpool3x3s1_fwd" in names and "avgpool3x3s1_bwd" in names
    inf = signature(NetworkV2(128, allocate=False, device="cpu", config={"repeat": [1, 1, 1]}), 6, False)
    assert "dropout_fwd" not in [op[0] for op in inf]
    no_drop = signature(NetworkV2(128, allocate=False, device="cpu", config={"repeat": [1, 1, 1], "keep_probability": 1.0}), 6, True)
    assert not any(op[0].startswith("dropout") for op in no_drop)


def test_v1_launch_lists_unchanged():
    """v1 plans (training + backward, inference layer-wise and with fused blocks) lower to the same launches with the same
    arguments as before the v2 refactor (tests/golden/v1_plan_signature.json, recorded on the previous engine)."""
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    for key, N, tr, E in (("train_triplet_6_E128", 6, True, 128), ("infer_6_E512", 6, False, 512), ("infer_32_E128", 32, False, 128)):
        sig = signature(Network(E, allocate=False, device="cpu"), N, tr)
        assert len(sig) == golden[key]["ops"], key
        assert hashlib.sha256(json.dumps(sig, sort_keys=True).encode()).hexdigest() == golden[key]["sha256"], key
