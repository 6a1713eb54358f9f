"""CPU checks of the autotuner policy and the attribution knobs' parsing (ops/tuning.py,
ops/conv_hip.py): without a GPU the tuner never times anything, returns the default and caches
it; the weight-gradient candidate whitelist parses ranges and lists."""
from simclr_amd.ops import conv_hip, tuning


def test_pick_without_gpu_returns_default_and_caches():
    calls = []
    key = ("test-tuning-default",)
    tuning._CACHE.pop(key, None)
    v = tuning.pick(key, [2, 4, 6], 4, lambda c: calls.append(c))
    assert v == 4 and calls == []
    assert tuning.cached(key) == 4
    # a cached key returns before the candidate list is even looked at
    assert tuning.pick(key, [], 9, lambda c: calls.append(c)) == 4
    tuning._CACHE.pop(key, None)


def test_pick_default_outside_candidates_falls_back_to_first():
    key = ("test-tuning-first",)
    tuning._CACHE.pop(key, None)
    assert tuning.pick(key, [3, 5], 7, lambda c: None) == 3
    tuning._CACHE.pop(key, None)


def test_pinned_choice_is_taken_only_while_admissible(tmp_path, monkeypatch):
    monkeypatch.setattr(tuning, "_CACHE", {})
    monkeypatch.setattr(tuning, "_PINNED", {})
    monkeypatch.setattr(tuning, "ENABLED", True)
    k1, k2 = ("igemm", (8, 4, 2), True, None, "x"), ("wgrad", (3,))
    tuning._CACHE.update({k1: 6, k2: 1})
    path = tmp_path / "tiles.json"
    assert tuning.save_table(path) == 2
    tuning._CACHE.clear()
    assert tuning.load_pinned(path) == 2 and tuning._PINNED == {k1: 6, k2: 1}
    calls = []
    assert tuning.pick(k1, [2, 4, 6], 4, calls.append) == 6 and calls == []
    assert tuning.cached(k1) == 6 and tuning.pinned_used() == 1
    # the pinned variant is not among the candidates any more: the usual policy decides
    assert tuning.pick(k2, [0, 2], 2, calls.append) == 2 and calls == []
    assert tuning.pinned_used() == 1
    # pins dropped: the usual policy again (no GPU here: the default)
    tuning.unpin()
    assert tuning.table() == {} and tuning.pick(k1, [2, 4, 6], 4, calls.append) == 4
    # the fixed-tile policy (runtime.deterministic) ignores pins
    tuning.pin({k1: 6})
    tuning.set_enabled(False)
    assert tuning.pick(k1, [2, 4, 6], 4, calls.append) == 4


def test_committed_bench_tiles_are_well_formed(monkeypatch):
    import json
    from pathlib import Path
    monkeypatch.setattr(tuning, "_PINNED", {})
    path = Path(__file__).resolve().parents[1] / "bench" / "tiles_mi355x.json"
    rows = json.loads(path.read_text())
    assert tuning.load_pinned(path) == len(rows) == len(tuning._PINNED) > 0
    for k, v in tuning._PINNED.items():
        assert isinstance(k, tuple) and k[0] in ("igemm", "wgrad", "wgrad1split"), k
        assert isinstance(v, int) and v >= 0
        hash(k)


def test_rounds_default():
    assert tuning.ROUNDS >= 1
