"""The host half of the 3x3 convolution families decides what it decided when tests/golden/conv_host_decisions.json was
recorded (tools/record_conv_host_decisions.py): bank and workspace sizes, split-K factors and routing answers over a grid of
ordinary and degenerate shapes, under three batch hints and the planner's tuning constants at and away from their defaults,
and the return code and message of every refused launch.  Pure host code: no GPU is needed or used."""
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (os.path.join(REPO, "tools"), os.path.join(REPO, "maua-style_amd")) if p not in sys.path]

import record_conv_host_decisions as rec  # noqa: E402


@pytest.fixture(scope="module")
def tables():
    import hip
    L = hip.lib()
    names = [t[0] for t in rec.TUNINGS]
    before = {k: L.maua_get_tuning(k.encode(), -12345.0) for k in names}, L.maua_get_split_batch_hint()
    now = rec.compute(L)
    after = {k: L.maua_get_tuning(k.encode(), -12345.0) for k in names}, L.maua_get_split_batch_hint()
    assert after == before, "the recorder left a tuning constant or the batch hint changed"
    with open(rec.GOLDEN) as f:
        return json.load(f), json.loads(json.dumps(now))


def test_every_query_answers_as_recorded(tables):
    want, got = tables
    assert got["shapes"] == want["shapes"] and got["channel_pairs"] == want["channel_pairs"]
    assert sorted(got["index"]) == sorted(want["index"])
    wrong = []
    for key in want["index"]:
        w, g = want["vectors"][want["index"][key]], got["vectors"][got["index"][key]]
        if w != g:
            if isinstance(w, dict) and isinstance(g, dict):
                blocks = [i for i, (a, b) in enumerate(zip(w["sha1"], g["sha1"])) if a != b]
                wrong.append(f"{key}: blocks of 256 shapes that differ: {blocks[:8]}")
            else:
                wrong.append(f"{key}: recorded {str(w)[:200]} now {str(g)[:200]}")
    assert not wrong, "\n".join(wrong[:20])


def test_every_refusal_is_as_recorded(tables):
    want, got = tables
    assert got["rejections_elsewhere"] == {} and want["rejections_elsewhere"] == {}, "a refusal depends on the planner's state"
    assert sorted(got["rejections"]) == sorted(want["rejections"])
    wrong = {k: (want["rejections"][k], got["rejections"][k]) for k in want["rejections"] if want["rejections"][k] != got["rejections"][k]}
    assert not wrong, wrong
    # refused by the argument checks (negative codes), not by a launch that failed
    assert all(rc < 0 and text for rc, text in got["rejections"].values())
    for entry in ("maua_conv3x3_x6", "maua_conv3x3_x3", "maua_conv3x3_x3w", "maua_conv3x3_x3w_relu_pool", "maua_conv3x3_x3w_gram",
                  "maua_conv3x3_x3w_unpool", "maua_conv3x3_x3q", "maua_conv3x3_x3q_relu_pool", "maua_conv3x3_x3q_unpool", "maua_conv3x3_x3p",
                  "maua_conv_kxk_x3", "maua_conv_pack_filters_x6", "maua_conv_pack_filters_x3", "maua_conv_pack_filters_x3w",
                  "maua_conv_pack_filters_x3q", "maua_conv_pack_filters_kxk_x3", "maua_conv2d_fwd", "maua_conv2d_bwd_data"):
        # (the filter packers have one refusal, "bad args"; every other entry point refuses for several reasons)
        assert len({tuple(v) for k, v in got["rejections"].items() if k.startswith(entry + ":")}) >= (1 if "pack_filters" in entry else 2), entry


def test_the_table_is_not_vacuous(tables):
    """Every recorded query takes at least two distinct values over the table (a grid of small ragged planes alone leaves
    maua_conv_x3q_preferred at 0 everywhere), and every tuning state moves at least one answer away from the defaults'."""
    want, _ = tables
    seen = {}
    for key, i in want["index"].items():
        v = want["vectors"][i]
        values = seen.setdefault(key.split("|")[2].split("/")[0], set())  # (a function asked with several filter sizes is one query)
        values.update(range(v["distinct"]) if isinstance(v, dict) else v[0::2])
    flat = {q: vals for q, vals in seen.items() if len(vals) < 2}
    assert not flat, flat
    for label, _, _ in rec.states()[1:]:  # (identical vectors are stored once: another index is another vector)
        moved = [q for q in rec.QUERIES if any(want["index"][f"{label}|{h}|{q}"] != want["index"][f"default|{h}|{q}"] for h in rec.HINTS)]
        assert moved or label.startswith("x3p_groups="), label  # (x3p_groups sizes the launch's grid: no query reads it)


def test_the_routing_queries_prefer_what_they_were_measured_to_prefer():
    import hip
    L = hip.lib()
    hint = L.maua_get_split_batch_hint()
    L.maua_set_split_batch_hint(1)
    try:
        assert L.maua_conv_x3q_preferred(1, 512, 128, 128, 512, 1) == 1 and L.maua_conv_x3q_preferred(1, 512, 90, 90, 512, 1) == 0
        assert L.maua_conv_x3p_preferred(1, 256, 256, 256, 256, 1) == 1
    finally:
        L.maua_set_split_batch_hint(hint)
