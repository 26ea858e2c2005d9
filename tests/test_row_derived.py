"""The derived word of a device table row (CPU; csrc/ge_layout.h DevRow r6, filled by csrc/ge_host.h ww8_row_derived).

A Werewolf row of a segment of at most 8 players carries, in the word that was the unused third permute selector, the constants
of the row that the fused lone-wavefront turn used to work out of r0 on every turn (ge_device.h ww_turn):
  bits 0..7    the all-players mask if the row completes by actions, else 0
  bit 8        the row's action is a night action (wolf target, Doctor, Detective)
  bits 16..23  the flags byte of a room that has left the row: phase-0-done | the row's effect << 1
  bits 28..31  the action kind one-hot, (1 << act) >> 1 (bit 28 wolf target .. bit 31 day vote)
Here: for every row of every committed DSL and every grammar variant, at 4, 8 and 12 players, the word is what the decoded
`completion`, `act` and `effect` of GameTable.rows() imply; every other layout keeps its third selector (a permute selector:
every byte at most 0x0D); r0 still decodes to the same fields; and rows() is, table by table, what it was before the word
existed (tests/golden/table_rows.json, recorded from the library without it)."""
import json
import os

import pytest

from conftest import GOLD, load_dsl
from game_engine_amd import GameTable, GeError
from oracle import dsl_variants

COMP_ACTION, ACT_WOLF_TARGET, ACT_DETECTIVE, PACK_WEREWOLF = 2, 1, 3, 1


def _tables():
    out = []
    for f in sorted(os.listdir(os.path.join(GOLD, "dsl"))):
        out.append(("dsl/" + f[:-5], f[:-5], None, 1))
    for name in sorted(dsl_variants.VARIANTS):
        game, builder, rounds = dsl_variants.VARIANTS[name]
        out.append(("variant/" + name, game, builder, rounds))
    return out


TABLES = _tables()


def _table(game, builder, rounds):
    dsl = load_dsl(game)
    return GameTable(builder(dsl) if builder else dsl, rounds)


def _expected(row, n_players):
    act = row["act"]
    night = ACT_WOLF_TARGET <= act <= ACT_DETECTIVE
    return (((1 << n_players) - 1 if row["completion"] == COMP_ACTION else 0) | (int(night) << 8) |
            ((1 | (row["effect"] << 1)) << 16) | ((((1 << act) >> 1) << 28) & 0xFFFFFFFF))


def test_every_table_is_listed():
    assert len(TABLES) >= 7 and sum(1 for t in TABLES if t[0].startswith("dsl/")) == 3


@pytest.mark.parametrize("n_players", [4, 8, 12])
@pytest.mark.parametrize("key,game,builder,rounds", TABLES, ids=[t[0] for t in TABLES])
def test_derived_word_is_what_the_decoded_fields_imply(key, game, builder, rounds, n_players):
    tb = _table(game, builder, rounds)
    rows = tb.rows()
    assert len(rows) == tb.n_phases >= 1
    for i, row in enumerate(rows):
        d = tb.dev_row(n_players, i)
        assert len(d) == 8
        # r0 as documented: completion [1:0], act [4:2], effect [7:5], n_branches [13:11]; nothing above bit 26
        assert (d[0] & 3, (d[0] >> 2) & 7, (d[0] >> 5) & 7, (d[0] >> 11) & 7) == (row["completion"], row["act"], row["effect"], len(row["branches"]))
        assert d[0] >> 27 == 0
        if tb.pack == PACK_WEREWOLF and n_players <= 8:
            assert d[6] == _expected(row, n_players), f"{key}, {n_players} players, row {i}: {d[6]:#010x} != {_expected(row, n_players):#010x}"
            # the four parts one by one, as the turn reads them
            assert d[6] & 0xFF == (((1 << n_players) - 1) if row["completion"] == COMP_ACTION else 0)
            assert (d[6] >> 8) & 1 == int(row["act"] in (1, 2, 3)) and (d[6] >> 9) & 0x7F == 0
            assert (d[6] >> 16) & 0xFF == 1 | (row["effect"] << 1) and (d[6] >> 24) & 0xF == 0
            assert d[6] >> 28 == ((1 << row["act"]) >> 1) & 0xF
        else:
            # the third permute selector of the wider layouts, as before: byte selectors 0..7 or the constant 0xFF (0x0D)
            assert all(((d[6] >> (8 * b)) & 0xFF) <= 0x0D for b in range(4)), f"{key}, {n_players} players, row {i}: {d[6]:#010x}"


def test_one_hot_kinds_of_the_shipped_game():
    tb = GameTable(load_dsl("werewolf-(mafia)"))
    kinds = {r["act"]: tb.dev_row(8, i)[6] >> 28 for i, r in enumerate(tb.rows())}
    assert kinds[0] == 0 and {kinds[a] for a in (1, 2, 3, 4)} == {1, 2, 4, 8}


def test_arguments_are_checked():
    tb = GameTable(load_dsl("werewolf-(mafia)"))
    for n, row in ((3, 0), (13, 0), (8, tb.n_phases), (8, 1 << 20)):
        with pytest.raises(GeError):
            tb.dev_row(n, row)


@pytest.mark.parametrize("key,game,builder,rounds", TABLES, ids=[t[0] for t in TABLES])
def test_rows_are_what_they_were(key, game, builder, rounds):
    with open(os.path.join(GOLD, "table_rows.json"), encoding="utf-8") as f:
        want = json.load(f)[key]
    got = json.loads(json.dumps(_table(game, builder, rounds).rows(), ensure_ascii=False))      # tuples -> lists, as the fixture holds them
    assert got == want
