"""SeatEnv - a resident RoomBatch as an environment for a decision maker that lives on the GPU and sits in a seat of every room
(POLICY.md §3n): observations and actions are torch tensors on the batch's device, every call goes on torch's current stream, and
no byte crosses to the host.  torch is imported when a SeatEnv is made; the rest of the package imports without it.  A process
that uses SeatEnv imports torch before it creates its first GameTable or RoomBatch: torch ships a HIP runtime of its own, and
the library binds to the runtime that is loaded first.

    env = SeatEnv(batch, seats=[1])
    obs = env.observe()
    for _ in range(steps):
        actions = SeatEnv.random_legal(obs)              # or a policy network's choice among fields(obs)["legal"]
        obs, done, won = env.step(actions)

A teacher for the loop (POLICY.md §3o): env.teach(64) fills `advice` with the playout advice of every listed seat - the win odds of
each choice it can make now - without leaving the device, and advice_fields(advice)["best"] is an action tensor for step().

A room that has ended shows done = 1 once at one turn per step; under restart=True the next step recycles it (the turn that starts
from a terminal phase re-initialises the room), so the observation after that step is of the new game.  step(actions, n) with
n > 1 fuses its turns: under restart=True a game that ends inside the call is recycled inside it as well, and its done and won are
never observed.  step_until is the call that shows every end (POLICY.md §3p): each room plays on until a listed seat must act, its
game has ended or the turn limit, so every observation is a decision point, a finished game or the limit -

        obs, done, won = env.step_until(actions)         # env.played: the turns each room took, env.stopped: why it stopped

Where the learner sits in every seat (self-play: all seats listed and host-driven), most entries of the [R, S] grid are no decision
point.  decisions() / step_decisions() work on a decision list instead (POLICY.md §3q): only the entries that are due, in entry
order, with their observations -

    dec_obs, dec_entries, dec_n = env.decisions()
    for _ in range(steps):
        choices = SeatEnv.random_legal(dec_obs)          # over all cap rows: no mask, the list's length stays on the device
        dec_obs, dec_entries, dec_n = env.step_decisions(choices)"""
from typing import Dict, Sequence

from .stepper import RoomBatch, ADVICE_BYTES
from ._lib import SEAT_OBS_BYTES

# byte offsets inside a ge_seat_obs (include/ge_step.h)
_BYTE_FIELDS = {"seat": 0, "n_players": 1, "pack": 2, "act": 3, "phase_row": 4}
_INT_FIELDS = {"phase_id": 0, "prev_phase_id": 1, "end_turn": 2, "games": 3}      # the four int32 from byte 12 on
# the four int32 a ge_advice begins with; behind them 13 ge_advice_option of 16 bytes: the policy's, then option[12]
_ADVICE_HEAD = {"status": 0, "legal_bits": 1, "best": 2, "phase_id": 3}


class SeatEnv:
    """Owns `obs` (uint8 [R, S, 192]: one ge_seat_obs per room and listed seat), `actions` and `status` (int32 [R, S]) on the
    batch's device, and `advice` (uint8 [R, S, 224]: one ge_advice each) from the first teach() on; R = batch.n_rooms,
    S = len(seats); from the first decisions() on the decision list as well: `dec_obs` (uint8 [cap, 192]), `dec_entries`,
    `dec_choices`, `dec_status` (int32 [cap]) and `dec_n` (int32 [2]).  The human mask and the seat plane play no part: to keep the policy from playing a listed seat as well, make
    it host-driven in the batch (human_mask / set_seats)."""

    def __init__(self, batch: RoomBatch, seats: Sequence[int]):
        import torch
        if not torch.cuda.is_available():
            # torch ships a HIP runtime of its own; one process can drive the GPU through one runtime only, and the library
            # binds to whichever is loaded first
            raise RuntimeError("SeatEnv: torch sees no GPU.  Import torch before the first GameTable / RoomBatch of the process, "
                               "so that libge_step.so and torch share one HIP runtime")
        self.batch, self.seats = batch, [int(s) for s in seats]
        self._torch = torch
        dev = torch.device("cuda", batch.device)
        shape = (batch.n_rooms, len(self.seats))
        self.obs = torch.zeros(shape + (SEAT_OBS_BYTES,), dtype=torch.uint8, device=dev)
        self.actions = torch.zeros(shape, dtype=torch.int32, device=dev)
        self.status = torch.zeros(shape, dtype=torch.int32, device=dev)
        self.advice = None                                   # uint8 [R, S, 224], made by the first teach()
        self.played = self.stopped = None                    # int32 [R], made by the first step_until() / step_decisions()
        self.dec_obs = self.dec_entries = self.dec_n = None  # the decision list, made by the first decisions()
        self.dec_choices = self.dec_status = None            # int32 [cap], beside it

    def _stream(self) -> int:
        return int(self._torch.cuda.current_stream(self.obs.device).cuda_stream)

    def _act(self, actions, st: int):
        torch = self._torch
        a = actions
        if not (a.dtype == torch.int32 and a.device == self.obs.device and a.is_contiguous() and a.shape == self.actions.shape):
            self.actions.copy_(a.reshape(self.actions.shape))
            a = self.actions
        self.batch.act_seats(self.seats, a, self.status, stream=st)

    def observe(self):
        """The observation tensor, filled for the batch as it stands."""
        self.batch.observe_seats(self.seats, self.obs, stream=self._stream())
        return self.obs

    def step(self, actions, n_turns: int = 1):
        """act_seats(actions), batch.step(n_turns), observe_seats - all on torch's current stream.  actions: [R, S] choices, 0 = no
        action (any integer dtype or device; an int32 tensor on the batch's device is read where it lies); `status` holds each
        entry's verdict afterwards.  Returns (obs, done, won): done and won are bool views [R, S] of the observation.  With
        n_turns > 1 the turns are fused: a room that waits for a listed seat idles, and a finished room stays finished unless
        the batch restarts, so step(actions, 16) is "play on until my seats are needed", within 16 turns - without restart
        only: a restarting batch recycles a game that ends inside the call, and step_until is the call to use."""
        st = self._stream()
        self._act(actions, st)
        self.batch.step(n_turns, stream=st)
        self.batch.observe_seats(self.seats, self.obs, stream=st)
        f = self.fields(self.obs)
        return self.obs, f["done"], f["won"]

    def step_until(self, actions, max_turns: int = 16, until=("seat", "end")):
        """act_seats(actions), batch.run_seats(max_turns, until), observe_seats - all on torch's current stream (POLICY.md §3p).
        Every room plays on until a listed seat is a pending target ("seat"), its game has ended ("end") or max_turns turns are
        played, so no end is lost under restart=True: a finished room is observed with done = 1 and recycled by the next call's
        first turn.  `until` as RoomBatch.run_seats takes it.  Returns (obs, done, won) as step(); `played` and `stopped` (int32
        [R], allocated on first use) hold the turns each room took and the RUN_SEATS_UNTIL bits that stopped it (0: the limit).
        The batch's turn advances by max_turns per call."""
        if self.played is None:
            torch = self._torch
            self.played = torch.zeros(self.batch.n_rooms, dtype=torch.int32, device=self.obs.device)
            self.stopped = torch.zeros(self.batch.n_rooms, dtype=torch.int32, device=self.obs.device)
        st = self._stream()
        self._act(actions, st)
        self.batch.run_seats(self.seats, self.played, self.stopped, max_turns, until, stream=st)
        self.batch.observe_seats(self.seats, self.obs, stream=st)
        f = self.fields(self.obs)
        return self.obs, f["done"], f["won"]

    def decisions(self, cap=None, want=("seat", "end")):
        """The decision list of the batch as it stands (RoomBatch.gather_seats, POLICY.md §3q), on torch's current stream: of the
        R * S entries of `obs`, those that are due - a listed seat that must act ("seat": legal != 0) or whose game has ended
        ("end": done) - in ascending entry order.  Returns (dec_obs, dec_entries, dec_n): dec_obs uint8 [cap, 192], the due
        records; dec_entries int32 [cap], their entry indices r * S + j; dec_n int32 [2], the number of rows filled and the
        number of due entries (they differ when cap is too small).  All three are allocated on first use, and again when cap
        changes; cap defaults to R * S, which always holds the whole list.
        Rows at and beyond dec_n[0] hold stale bytes - earlier lists' records, or zeros - never anything of this list.  A caller
        that runs its network over all cap rows need not mask them: step_decisions hands dec_n to act_listed, which reads it on
        the device and ignores every row behind the list.  fields() and random_legal() work on dec_obs as on obs.  teach() has
        no list form: index the dense `advice` with dec_entries."""
        torch = self._torch
        cap = self.actions.numel() if cap is None else int(cap)
        if self.dec_obs is None or self.dec_obs.shape[0] != cap:
            dev = self.obs.device
            self.dec_obs = torch.zeros((cap, SEAT_OBS_BYTES), dtype=torch.uint8, device=dev)
            self.dec_entries = torch.zeros(cap, dtype=torch.int32, device=dev)
            self.dec_choices = torch.zeros(cap, dtype=torch.int32, device=dev)
            self.dec_status = torch.zeros(cap, dtype=torch.int32, device=dev)
            self.dec_n = torch.zeros(2, dtype=torch.int32, device=dev)
        self._dec_want = want
        self.batch.gather_seats(self.seats, self.dec_obs, self.dec_entries, self.dec_n, want, cap=cap, stream=self._stream())
        return self.dec_obs, self.dec_entries, self.dec_n

    def step_decisions(self, choices, max_turns: int = 16, until=("seat", "end")):
        """act_listed(choices) with the list the last decisions() / step_decisions() left, batch.run_seats(max_turns, until),
        gather_seats - all on torch's current stream (POLICY.md §3q): step_until() for a learner that sits in many seats and
        looks only at those that are due.  choices: [cap] (any integer dtype or device; an int32 tensor on the batch's device is
        read where it lies), choices[i] for the entry dec_entries[i], 0 = no action; rows at and beyond dec_n[0] are ignored on
        the device, whatever they hold.  `dec_status` (int32 [cap]) holds each listed entry's verdict afterwards, `played` and
        `stopped` what step_until() leaves there.  The new list is gathered under the `want` of the last decisions().  Returns
        (dec_obs, dec_entries, dec_n) as decisions()."""
        if self.dec_obs is None:
            raise RuntimeError("SeatEnv.step_decisions: call decisions() first")
        torch = self._torch
        if self.played is None:
            self.played = torch.zeros(self.batch.n_rooms, dtype=torch.int32, device=self.obs.device)
            self.stopped = torch.zeros(self.batch.n_rooms, dtype=torch.int32, device=self.obs.device)
        c = choices
        if not (c.dtype == torch.int32 and c.device == self.obs.device and c.is_contiguous() and c.shape == self.dec_entries.shape):
            self.dec_choices.copy_(c.reshape(self.dec_entries.shape))
            c = self.dec_choices
        st = self._stream()
        cap = self.dec_entries.shape[0]
        self.batch.act_listed(self.seats, self.dec_n, self.dec_entries, c, self.dec_status, cap=cap, stream=st)
        self.batch.run_seats(self.seats, self.played, self.stopped, max_turns, until, stream=st)
        self.batch.gather_seats(self.seats, self.dec_obs, self.dec_entries, self.dec_n, self._dec_want, cap=cap, stream=st)
        return self.dec_obs, self.dec_entries, self.dec_n

    def teach(self, n_rollouts: int, max_turns: int = 1024, key0: int = 0, full_view: bool = False):
        """The playout advice of every listed seat for the batch as it stands (RoomBatch.teach_seats, POLICY.md §3o), on torch's
        current stream: `advice`, uint8 [R, S, 224], one ge_advice per room and listed seat, allocated on first use.  Room r is
        played under the key key0 + (r << 20), the batch's turn and the batch's seed.  advice_fields(advice)["best"] is an action
        tensor for step(): 0 exactly where nothing is legal."""
        if self.advice is None:
            self.advice = self._torch.zeros(self.actions.shape + (ADVICE_BYTES,), dtype=self._torch.uint8, device=self.obs.device)
        self.batch.teach_seats(self.seats, self.advice, n_rollouts, max_turns, key0=key0, full_view=full_view, stream=self._stream())
        return self.advice

    @staticmethod
    def advice_fields(advice) -> Dict[str, "object"]:
        """The fields of an advice tensor [..., 224] as tensor views (no copies): status, legal_bits, best, phase_id (int32);
        policy_finished, policy_wins (int32) and policy_score (int64), the entry without an action; finished, wins (int32) and
        score (int64) as [..., 12], index c-1 = choice c, zero where bit c-1 of legal_bits is clear."""
        import torch
        head = advice[..., 0:16].view(torch.int32)
        out = {name: head[..., at] for name, at in _ADVICE_HEAD.items()}
        out["policy_finished"] = advice[..., 16:20].view(torch.int32)[..., 0]
        out["policy_wins"] = advice[..., 20:24].view(torch.int32)[..., 0]
        out["policy_score"] = advice[..., 24:32].view(torch.int64)[..., 0]
        opt = advice[..., 32:224].unflatten(-1, (12, 16))
        out["finished"] = opt[..., 0:4].view(torch.int32)[..., 0]
        out["wins"] = opt[..., 4:8].view(torch.int32)[..., 0]
        out["score"] = opt[..., 8:16].view(torch.int64)[..., 0]
        return out

    @staticmethod
    def fields(obs) -> Dict[str, "object"]:
        """The fields of an observation tensor [..., 192] as tensor views (no copies): seat, n_players, pack, act, phase_row (uint8);
        done, won (bool); legal_bits, unknown (int16 bit masks: bit c-1 = choice c / bit i = seat i+1); phase_id, prev_phase_id,
        end_turn, games (int32); players [..., 12, 12] and det [..., 12] (uint8).  `legal` is the one derived tensor: legal_bits
        expanded to bool [..., 12], legal[..., c-1] = choice c would be accepted now."""
        import torch
        out = {name: obs[..., at] for name, at in _BYTE_FIELDS.items()}
        out["done"] = obs[..., 5].view(torch.bool)
        out["won"] = obs[..., 6].view(torch.bool)
        masks = obs[..., 8:12].view(torch.int16)
        out["legal_bits"], out["unknown"] = masks[..., 0], masks[..., 1]
        ints = obs[..., 12:28].view(torch.int32)
        for name, at in _INT_FIELDS.items():
            out[name] = ints[..., at]
        out["players"] = obs[..., 32:176].unflatten(-1, (12, 12))
        out["det"] = obs[..., 176:188]
        bit = torch.arange(12, device=obs.device, dtype=torch.int32)
        out["legal"] = ((out["legal_bits"].to(torch.int32).unsqueeze(-1) >> bit) & 1).bool()
        return out

    @staticmethod
    def random_legal(obs, generator=None):
        """A uniform legal choice per entry (int32, the shape of obs without its last axis), 0 where nothing is legal; computed on
        the device: the largest of twelve uniform draws among the legal choices."""
        import torch
        legal = SeatEnv.fields(obs)["legal"]
        draws = torch.rand(legal.shape, device=obs.device, generator=generator)
        pick = torch.where(legal, draws, torch.full_like(draws, -1.0)).argmax(dim=-1).to(torch.int32) + 1
        return torch.where(legal.any(dim=-1), pick, torch.zeros_like(pick))
