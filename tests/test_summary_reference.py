"""The summary reference (oracle/summary.py) on CPU: its packer == the product's view_to_words (csrc/ge_host.h, built with
g++ through tests/native/pack_words.cpp) for every record layout and player count, and its summary words == a scalar
restatement of include/ge_step.h's definitions.  A change of a packed layout fails here before any GPU sees it."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_dsl
from game_engine_amd.stepper import ROOM_VIEW_DTYPE
from oracle import dsl_table as T
from oracle import summary as S
from oracle.oracle import ROOM_DTYPE

GAMES = [("werewolf-(mafia)", 1), ("two-truths-and-a-lie", 1), ("two-truths-and-a-lie", 3), ("draft-werewolf-(mafia)", 1)]


@pytest.fixture(scope="module")
def pack_words(tmp_path_factory):
    exe = tmp_path_factory.mktemp("native") / "pack_words"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "pack_words.cpp"),
                           os.path.join(ROOT, "game_engine_amd", "csrc", "ge_table.cpp")])
    return str(exe)


def random_views(table, n, R, rng):
    """Random canonical views of any field value the record can hold, garbage in the absent seats (which no record keeps)."""
    v = np.zeros(R, dtype=ROOM_VIEW_DTYPE)
    ids = np.array([p.id for p in table.phases])
    v["phase_id"] = ids[rng.integers(0, len(ids), R)]
    v["prev_phase_id"] = ids[rng.integers(0, len(ids), R)]
    v["phase0_done"] = rng.integers(0, 2, R)
    v["end_turn"] = np.where(rng.integers(0, 3, R) == 0, -1, rng.integers(0, 0xFFFF, R))
    v["games"] = rng.integers(0, 0x10000, R)
    v["n_players"], v["pack"] = n, table.pack
    p = v["players"]
    p[:] = rng.integers(0, 256, p.shape)                             # absent seats: anything
    v["det"] = rng.integers(0, 256, v["det"].shape)
    if table.pack == T.PACK_WEREWOLF:
        p[:, :n, 0] = rng.integers(0, 5, (R, n))
        p[:, :n, 1] = rng.integers(0, 3, (R, n))
        for f in (2, 3, 4, 5, 6, 7, 9):
            p[:, :n, f] = rng.integers(0, 2, (R, n))
        p[:, :n, 8] = rng.integers(0, 16, (R, n))
        p[:, :n, 10] = rng.integers(0, 16, (R, n))
        v["det"][:, :n] = rng.integers(0, 3, (R, n))
    else:
        for f in (0, 1, 3, 4, 6, 9):
            p[:, :n, f] = rng.integers(0, 2, (R, n))
        for f in (2, 5, 10):
            p[:, :n, f] = rng.integers(0, 4, (R, n))
        p[:, :n, 7] = rng.integers(0, 256, (R, n))
        p[:, :n, 8] = rng.integers(0, 16, (R, n))
    return v


def views_as_rooms(table, views):
    r = np.zeros(len(views), dtype=ROOM_DTYPE)
    idx = {p.id: p.idx for p in table.phases}
    r["phase"] = [idx[int(x)] for x in views["phase_id"]]
    r["prev"] = [idx[int(x)] for x in views["prev_phase_id"]]
    for f in ("phase0_done", "end_turn", "games", "det"):
        r[f] = views[f]
    r["n"], r["p"] = views["n_players"], views["players"]
    return r


@pytest.mark.parametrize("game,rounds", GAMES)
def test_packer_equals_view_to_words(pack_words, tmp_path, game, rounds):
    dsl = load_dsl(game)
    table = T.compile_dsl(dsl, rounds=rounds)
    dsl_path = tmp_path / "dsl.json"
    import json
    dsl_path.write_text(json.dumps(dsl, ensure_ascii=False), encoding="utf-8")
    kinds = set()
    for n in range(2, 13):
        rng = np.random.default_rng(n * 7 + rounds)
        views = random_views(table, n, 3000, rng)
        vin, wout = tmp_path / f"views{n}.bin", tmp_path / f"words{n}.bin"
        views.tofile(vin)
        subprocess.check_call([pack_words, str(dsl_path), str(rounds), str(n), str(vin), str(wout)])
        kind = S.kind_of(table.pack, n)
        kinds.add(kind)
        want = np.fromfile(wout, dtype="<u4").reshape(len(views), S.WORDS[kind])
        got = S.pack_records(kind, views_as_rooms(table, views), table)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert not len(bad), (f"{game} n={n}: {len(bad)} records differ; first room {bad[0]}: "
                              f"reference {[hex(x) for x in got[bad[0]]]} product {[hex(x) for x in want[bad[0]]]}")
    assert kinds == ({S.K_WW8, S.K_WW12} if table.pack == T.PACK_WEREWOLF else {S.K_TT4, S.K_TT8, S.K_TT12})


def _mix(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def _scalar_summary(table, n, rooms, records, first, turn):
    """include/ge_step.h ge_summary, one room at a time in Python integers."""
    w = [0] * S.SUMMARY_WORDS
    w[S.W_ROOMS], w[S.W_TURN] = len(rooms), turn
    for i, r in enumerate(rooms):
        fin = len(table.phases[int(r["phase"])].branches) == 0
        et = int(r["end_turn"])
        if fin:
            w[S.W_FINISHED] += 1
            if et >= 0:
                w[S.W_SUM_END] += et
                w[S.W_END_HIST + min(et // 8, 15)] += 1
        if table.pack == T.PACK_WEREWOLF:
            alive = [int(r["p"][k][2]) != 0 for k in range(n)]
            wolves = sum(1 for k in range(n) if alive[k] and int(r["p"][k][1]) == 2)
            w[S.W_ALIVE] += sum(alive)
            if fin:
                w[S.W_VILLAGE if wolves == 0 else S.W_WOLF] += 1
        else:
            w[S.W_ALIVE] += n
            for k in range(n):
                w[S.W_SCORE_HIST + min(int(r["p"][k][7]), 15)] += 1
        g = first + i
        h = _mix((g & 0xFFFFFFFF) ^ _mix((g >> 32) ^ 0xA5A5A5A5))
        for x in records[i]:
            h = _mix(h ^ int(x))
        w[S.W_CHECKSUM] = (w[S.W_CHECKSUM] + (h | _mix(h ^ 0x5BD1E995) << 32)) & 0xFFFFFFFFFFFFFFFF
        w[S.W_GAMES] += int(r["games"])
    return w


@pytest.mark.parametrize("game,n", [("werewolf-(mafia)", 7), ("werewolf-(mafia)", 11), ("two-truths-and-a-lie", 4),
                                    ("two-truths-and-a-lie", 8), ("two-truths-and-a-lie", 12)])
def test_summary_words_equal_scalar_definitions(game, n):
    """Every word from random rooms (terminal phases with and without an end_turn among them), segments split into parts
    and global indices past 2^32: the vectorised reference == the definitions one room at a time."""
    table = T.compile_dsl(load_dsl(game))
    rng = np.random.default_rng(n)
    views = random_views(table, n, 600, rng)
    terminal = [p.id for p in table.phases if not p.branches]
    views["phase_id"][::5] = terminal[0]                        # plenty of finished rooms, end_turn set or not
    rooms = views_as_rooms(table, views)
    first, turn = (1 << 32) - 300, 1234
    got = S.reference_summary_words([(table, n, rooms[:250]), (table, n, rooms[250:])], first, turn)
    want = _scalar_summary(table, n, rooms, S.pack_records(S.kind_of(table.pack, n), rooms, table), first, turn)
    assert [int(x) for x in got] == want
    fin_unset = sum(1 for r in rooms if not table.phases[int(r["phase"])].branches and int(r["end_turn"]) < 0)
    assert fin_unset > 0 and int(got[S.W_FINISHED]) > sum(int(x) for x in got[S.W_END_HIST:S.W_END_HIST + 16])
    part = S.reference_summary_words([(table, n, rooms[:250])], first, turn)
    rest = S.reference_summary_words([(table, n, rooms[250:])], first + 250, turn)
    with np.errstate(over="ignore"):
        both = part + rest
    both[S.W_TURN] = turn
    assert np.array_equal(both, got)                            # every field is a sum over rooms, mod 2^64


def test_checksum_depends_on_every_field_and_the_room_index():
    table = T.compile_dsl(load_dsl("werewolf-(mafia)"))
    rooms = views_as_rooms(table, random_views(table, 8, 1, np.random.default_rng(3)))
    base = S.reference_summary_words([(table, 8, rooms)], 5, 0)[S.W_CHECKSUM]
    assert S.reference_summary_words([(table, 8, rooms)], 6, 0)[S.W_CHECKSUM] != base
    for f in range(11):
        r = rooms.copy()
        r["p"][0, 0, f] = (int(r["p"][0, 0, f]) + 1) % (5 if f == 0 else 3 if f == 1 else 16 if f in (8, 10) else 2)
        assert S.reference_summary_words([(table, 8, r)], 5, 0)[S.W_CHECKSUM] != base, f
