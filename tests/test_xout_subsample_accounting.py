"""Algorithmic bytes of the two launches in front of a stride-2 subsample unit (arch.launch_algorithmic_bytes): X' is counted at the
pixels that are stored, [:, ::2, ::2], since the engine stores no others (DGP_XOUT_SUBSAMPLE).  Hand figures at the benchmark shape
(ResNet-50, 480 x 640, batch 32, 4 bytes per value); every other launch of the round-6 layer table keeps the figure it had
(tests/golden/r6_launch_algorithmic_bytes.json: the accounting before this change, per launch name of profiles/r6_layer_table_hipevents.tsv)."""
import json
import os

from deepgraphpose_amd.arch import launch_algorithmic_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B1 = "resnet_v1_50/block1/"
B2 = "resnet_v1_50/block2/"
UNIT = "conv:%sunit_2/bottleneck_v1/conv2+%sunit_2/bottleneck_v1/conv3+%sunit_3/bottleneck_v1/conv1|unit_c64_n64_id" % (B1, B1, B1)
CHAIN = "conv:%sunit_3/bottleneck_v1/conv3+%sunit_4/bottleneck_v1/conv1|chain_c128_n128_id" % (B2, B2)
N = 32


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "r6_launch_algorithmic_bytes.json")) as f:
        g = json.load(f)
    assert g["shape"] == {"h": 480, "w": 640, "depth": 50, "batch": N, "elem_bytes": 4.0}
    return g["bytes"]


def test_the_two_launches_count_the_kept_quarter_of_x_out():
    # block1 runs on 120 x 160 (C = 64, 4C = 256), block2 on 60 x 80 (C = 128, 4C = 512); weights as before: every panel once
    p1, k1 = N * 120 * 160, N * 60 * 80
    unit = 4.0 * (p1 * 64 + p1 * 256 + k1 * 256 + p1 * 64 + 9 * 64 * 64 + 64 * 256 + 256 * 64)      # R1 in, X in, X' kept, R1' out, w2, w3, w1'
    p2, k2 = N * 60 * 80, N * 30 * 40
    chain = 4.0 * (p2 * 128 + p2 * 512 + k2 * 512 + p2 * 128 + 128 * 512 + 512 * 128)               # R2 in, X in, X' kept, R1' out, w3, w1'
    got_u, got_c = launch_algorithmic_bytes(UNIT, 480, 640, 50, N), launch_algorithmic_bytes(CHAIN, 480, 640, 50, N)
    assert got_u == unit and got_c == chain
    assert abs(got_u / 1e6 - 1101.3) < 0.1 and abs(got_c / 1e6 - 551.1) < 0.1
    g = _golden()
    assert abs((g[UNIT] - got_u) / 1e6 - 471.9) < 0.1 and abs((g[CHAIN] - got_c) / 1e6 - 235.9) < 0.1      # the dead stores
    # the 16-bit tier's cells are half as large
    assert launch_algorithmic_bytes(UNIT, 480, 640, 50, N, 2.0) == unit / 2 and launch_algorithmic_bytes(CHAIN, 480, 640, 50, N, 2.0) == chain / 2


def test_every_other_launch_of_the_layer_table_is_unchanged():
    g = _golden()
    with open(os.path.join(ROOT, "profiles", "r6_layer_table_hipevents.tsv")) as f:
        names = [line.split("\t")[1] for line in f.read().splitlines()[1:]]
    assert len(names) == 43 and set(names) == set(g) and UNIT in g and CHAIN in g
    for n in names:
        if n not in (UNIT, CHAIN):
            assert launch_algorithmic_bytes(n, 480, 640, 50, N) == g[n], n
    total = sum(launch_algorithmic_bytes(n, 480, 640, 50, N) for n in names)
    assert abs((sum(g.values()) - total) / 1e9 - 0.708) < 5e-4


def test_odd_grids_count_ceil_halves_and_the_full_store_cases_stay():
    # 100 x 132 frames: block1 on 25 x 33 -> kept 13 x 17
    full = launch_algorithmic_bytes(UNIT, 100, 132, 50, 1) - 4.0 * 13 * 17 * 256 + 4.0 * 25 * 33 * 256
    lone = "conv:%sunit_2/bottleneck_v1/conv3|splith3_128x64_k32" % B1            # conv3 alone: unit_3's conv1 reads all of X'
    assert launch_algorithmic_bytes(lone, 100, 132, 50, 1) == 4.0 * (25 * 33 * (64 + 256 + 256) + 64 * 256)
    assert full == 4.0 * (25 * 33 * (64 + 256 + 256 + 64) + 9 * 64 * 64 + 64 * 256 + 256 * 64)
    # the first identity chain of block2 feeds a stride-1 unit: everything is stored
    first = "conv:%sunit_2/bottleneck_v1/conv3+%sunit_3/bottleneck_v1/conv1|chain_c128_n128_id" % (B2, B2)
    assert launch_algorithmic_bytes(first, 480, 640, 50, N) == _golden()[first]
