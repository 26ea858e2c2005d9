"""Oracle-side reference of ge_batch_step_rooms_playout (tests only): POLICY.md §3d restated on oracle ROOM_DTYPE records.
Who decides and from which candidates (steps 1-2) in Python; each candidate valued by rollout_seats_ref's entry (step 3); the
argmax with the pick(d, m) tie-break (step 4); then Oracle.inject and a 1-turn Oracle.run under the segment's human mask, with
the injected seats ORed into the turn's event (step 5)."""
from oracle.dsl_table import ACT_DAY_VOTE, ACT_DETECTIVE, ACT_DOCTOR_PROTECT, ACT_TT_STATEMENTS, ACT_WOLF_TARGET, COMP_ACTION
from oracle.rng import draw, pick, room_key, turn_key
from rollout_actions_ref import inject_all
from rollout_seats_ref import reference_rollout_seats

W_ROLE, W_TEAM, W_ALIVE = 0, 1, 2
ROLE_DETECTIVE, TEAM_WEREWOLVES = 4, 2
SEAT_WINS = 41 + 12                  # seat_wins[0] among the 77 words of ge_rollout_stats


def candidates(orc, room, seat: int):
    """The policy's candidate set of `seat` (1-based) in the room's current phase, ascending (POLICY.md §3 table)."""
    ph = orc.table.phases[int(room["phase"])]
    if orc.table.pack != 1:
        return [1] if ph.act == ACT_TT_STATEMENTS else [1, 2, 3]
    n, p, i = orc.n, room["p"], seat - 1
    alive = [j for j in range(n) if p[j][W_ALIVE]]
    wolf = [p[j][W_TEAM] == TEAM_WEREWOLVES for j in range(n)]
    if ph.act == ACT_WOLF_TARGET:
        cand = [j for j in alive if not wolf[j]]
    elif ph.act == ACT_DETECTIVE:
        cand = [j for j in alive if j != i and room["det"][j] == 0] or [j for j in alive if j != i]
    elif ph.act == ACT_DAY_VOTE:
        known = [j for j in alive if room["det"][j] == 2]
        if wolf[i]:
            cand = [j for j in alive if not wolf[j]]
        elif p[i][W_ROLE] == ROLE_DETECTIVE and known:
            cand = known[:1]
        else:
            cand = [j for j in alive if j != i]
    else:                                                    # ACT_DOCTOR_PROTECT
        cand = list(alive)
    return [j + 1 for j in (cand or alive)]


def seat_draw(seed: int, key: int, turn: int, seat: int) -> int:
    return draw(turn_key(room_key(seed, key), turn), seat - 1)


def due_seats(orc, room, seed: int, key: int, turn: int, restart: bool, human_mask: int):
    """The bots §1 step 1 makes act in this turn (1-based), or [] for a turn in which no playout decision is made."""
    ph = orc.table.phases[int(room["phase"])]
    if restart and not ph.branches:
        return []                                            # a restart-terminal turn
    if int(room["phase"]) == 0 and not room["phase0_done"]:
        return []                                            # the phase-0 guard
    if ph.completion != COMP_ACTION:
        return []
    out = []
    for s in range(1, orc.n + 1):
        if (human_mask >> (s - 1)) & 1 or seat_draw(seed, key, turn, s) & 3 == 0:
            continue
        if inject_all(orc, room, [(s, candidates(orc, room, s)[0])])[1] == 0:   # a living target that has not acted
            out.append(s)
    return out


def policy_choice(orc, room, seed: int, key: int, turn: int, seat: int) -> int:
    cand = candidates(orc, room, seat)
    return cand[pick(seat_draw(seed, key, turn, seat), len(cand))]


def decide(orc, room, seed: int, key: int, turn: int, mask: int, pkey: int, pseed: int, R: int, M: int, full_view: bool,
           restart: bool = False, human_mask: int = 0):
    """[(seat, choice)] of the playout seats that decide in this turn (ascending seat)."""
    out = []
    for s in due_seats(orc, room, seed, key, turn, restart, human_mask):
        if not (mask >> (s - 1)) & 1:
            continue
        cand = candidates(orc, room, s)
        if len(cand) < 2:
            continue
        vals = [int(reference_rollout_seats(orc, room, pseed, pkey, turn, 0 if full_view else s, [(s, c)], R, M)[0][SEAT_WINS + s - 1])
                for c in cand]
        tied = [c for c, v in zip(cand, vals) if v == max(vals)]
        out.append((s, tied[pick(seat_draw(seed, key, turn, s), len(tied))]))
    return out


def reference_step_playout(orc, rooms, i, seed: int, key: int, turn: int, mask: int, pkey: int, pseed: int, R: int, M: int,
                           full_view: bool = False, restart: bool = False, human_mask: int = 0):
    """Room i of `rooms` (oracle ROOM_DTYPE, changed in place) one turn with playout seats, the decided seats ORed into its
    ev_newly / ev_choice; returns the decided mask."""
    chosen = decide(orc, rooms[i], seed, key, turn, mask, pkey, pseed, R, M, full_view, restart, human_mask)
    one = rooms[i:i + 1].copy()
    for s, c in chosen:
        assert orc.inject(one, 0, s, c), (s, c)
    orc.run(one, seed, key, turn, 1, threads=1, restart=restart, human_mask=human_mask)
    dmask = 0
    for s, c in chosen:
        one[0]["ev_newly"] |= 1 << (s - 1)
        one[0]["ev_choice"][s - 1] = c
        dmask |= 1 << (s - 1)
    rooms[i] = one[0]
    return dmask
