"""Helpers shared by the GPU parity tests: oracle rooms -> the product's room-view layout."""
import numpy as np

from game_engine_amd.stepper import ROOM_VIEW_DTYPE


def oracle_rooms_as_views(orc, rooms: np.ndarray) -> np.ndarray:
    """oracle.oracle.ROOM_DTYPE array -> ROOM_VIEW_DTYPE array (vectorised), for whole-batch memcmp."""
    ids = np.array(orc.ids, dtype=np.int32)
    v = np.zeros(len(rooms), dtype=ROOM_VIEW_DTYPE)
    v["phase_id"] = ids[rooms["phase"]]
    v["prev_phase_id"] = ids[rooms["prev"]]
    v["end_turn"] = rooms["end_turn"]
    v["games"] = rooms["games"]
    v["phase0_done"] = rooms["phase0_done"]
    v["n_players"] = rooms["n"]
    v["pack"] = orc.table.pack
    v["players"] = rooms["p"]
    v["players"][:, :, 11] = 0
    v["det"] = rooms["det"]
    return v


def oracle_batch(orc, n_rooms, seed, first_room, turns, threads=0, restart=False):
    rooms = orc.init_rooms(n_rooms)
    orc.run(rooms, seed, first_room, 0, turns, threads=threads, restart=restart)
    return oracle_rooms_as_views(orc, rooms)


def assert_views_equal(got: np.ndarray, want: np.ndarray, what=""):
    if got.tobytes() == want.tobytes():
        return
    for name in ROOM_VIEW_DTYPE.names:
        bad = np.nonzero((got[name] != want[name]).reshape(len(got), -1).any(axis=1))[0]
        if len(bad):
            i = int(bad[0])
            raise AssertionError(f"{what}: field {name!r} differs in {len(bad)} rooms; first room {i}: "
                                 f"got {got[name][i].tolist()} want {want[name][i].tolist()}")
    raise AssertionError(what + ": padding differs")


def oracle_events(orc, rooms: np.ndarray, turn: int) -> np.ndarray:
    """The oracle's record of the turn it just ran, in the product's ge_turn_event layout."""
    from game_engine_amd.stepper import EVENT_DTYPE
    ids = np.array(orc.ids, dtype=np.int32)
    e = np.zeros(len(rooms), dtype=EVENT_DTYPE)
    e["turn"] = turn
    e["from_phase_id"] = ids[rooms["ev_from"]]
    e["to_phase_id"] = ids[rooms["ev_to"]]
    e["acted_now"] = rooms["ev_newly"]
    e["restarted"] = rooms["ev_restarted"]
    e["choice"] = rooms["ev_choice"]
    return e


def views_as_oracle_rooms(orc, views: np.ndarray) -> np.ndarray:
    """ROOM_VIEW_DTYPE array -> oracle ROOM_DTYPE array (inverse of oracle_rooms_as_views)."""
    from oracle.oracle import ROOM_DTYPE
    idx_of = {pid: i for i, pid in enumerate(orc.ids)}
    r = np.zeros(len(views), dtype=ROOM_DTYPE)
    r["phase"] = [idx_of[int(x)] for x in views["phase_id"]]
    r["prev"] = [idx_of[int(x)] for x in views["prev_phase_id"]]
    r["phase0_done"] = views["phase0_done"]
    r["n"] = views["n_players"]
    r["end_turn"] = views["end_turn"]
    r["games"] = views["games"]
    r["p"] = views["players"]
    r["det"] = views["det"]
    return r


def rendered_turn_calls(orc, table, case, restart=False):
    """For every turn of one golden case, stepped by the oracle: (turn, the tool calls game_engine_amd.toolcalls renders for
    it, whether the turn recycled the room).  A recycled room's calls are rendered from a fresh room, as a new thread's."""
    from game_engine_amd.toolcalls import turn_tool_calls
    rooms = orc.init_rooms(1)
    for t in range(len(case["turns"])):
        before = oracle_rooms_as_views(orc, rooms)[0].copy()
        orc.run(rooms, case["seed"], case["room"], t, 1, restart=restart)
        after = oracle_rooms_as_views(orc, rooms)[0]
        ev = oracle_events(orc, rooms, t)[0]
        if ev["restarted"]:
            before = oracle_rooms_as_views(orc, orc.init_rooms(1))[0]
        yield t, turn_tool_calls(table, before, after, ev), bool(ev["restarted"])


def calls_digest(calls) -> str:
    """A short, order-sensitive digest of one turn's tool calls (names and arguments)."""
    import hashlib
    import json
    return hashlib.sha256(json.dumps(calls, ensure_ascii=False, separators=(",", ":")).encode("utf-8")).hexdigest()[:16]


def assert_summary_equal(got, want, what=""):
    """Summaries as words (RoomBatch.summary_words / oracle.summary.reference_summary_words) or dicts, field by field."""
    from game_engine_amd.stepper import summary_to_dict
    g, w = (x if isinstance(x, dict) else summary_to_dict(np.asarray(x, dtype=np.uint64)) for x in (got, want))
    bad = {k: (g[k], w[k]) for k in g if g[k] != w[k]}
    assert not bad, f"{what}: summary fields differ (got, reference): {bad}"


def raw_records(batch, segment, n_rooms, words):
    """The packed records of a segment as they lie in HBM (ge_batch_state + a D2H copy), [n_rooms, words] uint32:
    plane j holds words 4j..4j+3 of every room (ge_layout.h)."""
    import ctypes as C
    batch.sync()
    ptr, nbytes, bpr = batch.state(segment)
    assert bpr == 4 * words
    raw = np.empty(nbytes, dtype=np.uint8)
    assert C.CDLL("libamdhip64.so").hipMemcpy(C.c_void_p(raw.ctypes.data), C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0
    planes = (words + 3) // 4
    padded = nbytes // (16 * planes)
    out = np.empty((n_rooms, words), dtype=np.uint32)
    for j in range(planes):
        pw = min(4, words - 4 * j)
        plane = raw[j * 16 * padded:(j + 1) * 16 * padded].view(np.uint32)[: padded * pw].reshape(padded, pw)
        out[:, 4 * j:4 * j + pw] = plane[:n_rooms]
    return out


def assert_records_canonical(batch, segment, orc, rooms, what=""):
    """Every raw record of the segment == the summary reference's canonical packing of the oracle's rooms (Werewolf x 8:
    the prepared-deal cache, word 7's upper half, aside) - no bit outside the view depends on which kernel wrote it."""
    from oracle.summary import WORDS, kind_of, pack_records, K_WW8
    kind = kind_of(orc.table.pack, orc.n)
    got = raw_records(batch, segment, len(rooms), WORDS[kind])
    if kind == K_WW8:
        got[:, 7] &= 0xFFFF
    want = pack_records(kind, rooms, orc.table)
    bad = np.nonzero((got != want).any(axis=1))[0]
    if len(bad):
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} raw records differ from the canonical packing; first room {i}: "
                             f"HBM {[hex(x) for x in got[i]]} canonical {[hex(x) for x in want[i]]}")


def oracle_summary_words(orc, n_rooms, seed, first, turns, restart=False, chunk=1 << 20, each=None):
    """The reference summary of n_rooms rooms of one game stepped by the oracle from the initial state, run chunk by chunk
    (rooms are independent and keyed by their global index).  each(lo, rooms) sees every chunk's oracle rooms."""
    from oracle.summary import SUMMARY_WORDS, W_TURN, add_rooms
    words = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
    for lo in range(0, n_rooms, chunk):
        rooms = orc.init_rooms(min(chunk, n_rooms - lo))
        orc.run(rooms, seed, first + lo, 0, turns, threads=0, restart=restart)
        add_rooms(words, orc.table, orc.n, rooms, first + lo)
        if each is not None:
            each(lo, rooms)
    words[W_TURN] = turns
    return words
