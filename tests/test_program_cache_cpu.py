"""ProgramCache (refiners_amd/engine/program.py): the one place the single-pass engines keep their rules for dropping, bounding, refusing and
sweeping.  Driven with stub lowerings (an empty step, so a Program is made and never run): no GPU."""
import warnings
from types import SimpleNamespace

import pytest

from refiners_amd.engine.packing import Unsupported
from refiners_amd.engine.program import MAX_PROGRAMS, Entry, ProgramCache


class _Builds:
    """build functions that pack under the given names, and a record of the keys that were really lowered."""

    def __init__(self) -> None:
        self.calls: list = []

    def __call__(self, tag, packs=(), error=None):
        def build(cache):
            self.calls.append(tag)
            for p in packs:
                cache.get((p,), lambda: p)
            if error is not None:
                raise error
            low = SimpleNamespace(step=[], stats={"fallback_nodes": []}, step_pool=SimpleNamespace(bytes=lambda: 0))
            return Entry(low=low, use_graph=False, tag=tag)

        return build


def _packs(pc: ProgramCache) -> set:
    return {k[0] for k in pc.cache.store}


def test_a_hit_returns_the_same_entry_without_building():
    pc, b = ProgramCache("Engine", MAX_PROGRAMS), _Builds()
    e = pc.get("v", "a", b("a"))
    assert pc.get("v", "a", b("a again")) is e and b.calls == ["a"] and pc.lowerings == 1
    assert e.program.ops is e.low.step and e.program.low is e.low and not e.program.use_graph and pc.last is e
    assert e.stats == {"fallback_nodes": [], "step_ops": 0, "pool_bytes": 0}


def test_a_version_change_drops_entries_refusals_and_use_marks():
    pc, b = ProgramCache("Engine", MAX_PROGRAMS, fallback=True), _Builds()
    pc.get("v", "a", b("a", ["wa"]))
    pc.get("v", "b", b("b", ["wb"]))
    with pytest.warns(RuntimeWarning):
        pc.get("v", "bad", b("bad", error=Unsupported("no")))
    assert len(pc.entries) == 2 and pc.refused == {"bad"} and pc.cache.used == {("wb",)}
    e = pc.get("w", "a", b("a2", ["wa"]))
    assert list(pc.entries) == ["a"] and e.tag == "a2" and not pc.refused and pc.version == "w" and pc.lowerings == 3
    assert _packs(pc) == {"wa"} and pc.cache.used == set()  # (the marks of "v" were cleared before "a2" made its own, and the sweep took those)


@pytest.mark.parametrize("capacity", [1, MAX_PROGRAMS])
def test_capacity_bounds_the_entries_oldest_first(capacity):
    pc, b = ProgramCache("Engine", capacity), _Builds()
    for k in range(capacity + 1):
        pc.get("v", k, b(k))
    assert list(pc.entries) == list(range(1, capacity + 1)) and pc.lowerings == capacity + 1
    pc.get("v", 0, b("0 again"))  # evicted: lowered again
    assert b.calls[-1] == "0 again" and list(pc.entries) == list(range(2, capacity + 1)) + [0]


def test_a_second_shape_does_not_sweep_the_first_shapes_packs():
    pc, b = ProgramCache("Engine", MAX_PROGRAMS), _Builds()
    pc.get("v", "a", b("a", ["shared", "wa"]))
    pc.get("v", "b", b("b", ["shared", "wb"]))
    assert _packs(pc) == {"shared", "wa", "wb"}
    # an edit: every program goes, and the first lowering after it sweeps what no live entry used
    pc.get("w", "b", b("b2", ["shared", "wb2"]))
    assert _packs(pc) == {"shared", "wb2"}
    pc.get("w", "a", b("a2", ["shared", "wa2"]))
    assert _packs(pc) == {"shared", "wb2", "wa2"}


def test_with_one_slot_every_lowering_sweeps():
    pc, b = ProgramCache("Engine"), _Builds()
    pc.get("v", "a", b("a", ["shared", "wa"]))
    pc.get("v", "b", b("b", ["shared", "wb"]))
    assert _packs(pc) == {"shared", "wb"} and list(pc.entries) == ["b"]
    pc.get("w", "b", b("b2", ["shared", "wb2"]))
    assert _packs(pc) == {"shared", "wb2"}


def test_a_lowering_after_a_refused_first_one_sweeps():
    pc, b = ProgramCache("Engine", MAX_PROGRAMS, fallback=True), _Builds()
    pc.get("v", "a", b("a", ["old"]))
    with pytest.warns(RuntimeWarning):
        assert pc.get("w", "bad", b("bad", ["half"], error=Unsupported("no"))) is None
    assert _packs(pc) == {"old", "half"} and not pc.entries
    pc.get("w", "a", b("a2", ["new"]))  # the only entry held: the stale pack goes now, not at the next edit
    assert _packs(pc) == {"half", "new"}


def _engine_call(pc, key, build):
    return pc.get("v", key, build)  # (stands for an engine's __call__)


def test_a_fallback_engine_warns_once_per_key_and_version():
    pc, b = ProgramCache("CompiledThing", MAX_PROGRAMS, fallback=True), _Builds()
    with pytest.warns(RuntimeWarning, match=r"^CompiledThing: odd tree; running the stock forward$") as rec:
        assert _engine_call(pc, "a", b("a", error=Unsupported("odd tree"))) is None  # the line the warning names
    assert rec[0].filename == __file__ and rec[0].lineno == test_a_fallback_engine_warns_once_per_key_and_version.__code__.co_firstlineno + 3
    assert pc.last is None and pc.lowerings == 0 and not pc.entries
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert pc.get("v", "a", b("a again")) is None and b.calls == ["a"]  # remembered: no second attempt, no second warning
        assert pc.get("v", "b", b("b")).tag == "b" and pc.last.tag == "b"
        assert pc.get("v", "a", b("a again")) is None and pc.last is None  # ... also behind another key's program
    with pytest.warns(RuntimeWarning, match="CompiledThing: still odd"):
        assert pc.get("w", "a", b("a retried", error=Unsupported("still odd"))) is None  # a version change retries
    assert b.calls == ["a", "b", "a retried"]


def test_a_strict_engine_lets_unsupported_through_and_remembers_nothing():
    pc, b = ProgramCache("Engine", MAX_PROGRAMS), _Builds()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for n in (1, 2):
            with pytest.raises(Unsupported, match="odd tree"):
                pc.get("v", "a", b("a", error=Unsupported("odd tree")))
            assert len(b.calls) == n and not pc.refused and not pc.entries and pc.lowerings == 0


@pytest.mark.parametrize("fallback", [False, True])
def test_other_errors_propagate_and_leave_the_cache_as_it_was(fallback):
    pc, b = ProgramCache("Engine", MAX_PROGRAMS, fallback=fallback), _Builds()
    kept = pc.get("v", "a", b("a"))
    with pytest.raises(RuntimeError, match="too small"):
        pc.get("v", "b", b("b", error=RuntimeError("too small")))
    assert pc.lowerings == 1 and pc.entries == {"a": kept} and not pc.refused
