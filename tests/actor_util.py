"""Shared by tests/test_actor_host.py and tests/test_gpu_actor.py: the designed
schedule of game ends for the episode bookkeeping, and the tallies of the
exploration process."""
import functools

import numpy as np

GAMES = 2
T_DESIGNED = 16


@functools.lru_cache(maxsize=None)
def schedule(n_env=6):
    """(reward float32 [T, N, 2], done uint8 [T, N]) of 16 ticks, two recorded
    games per env.  Envs 0..5 are written by hand (``EXPECT``); further envs end
    games at random with random rewards."""
    T, N = T_DESIGNED, int(n_env)
    rng = np.random.RandomState(11)
    done = np.where(rng.rand(T, N) < 0.2, rng.randint(1, 3, size=(T, N)), 0).astype(np.uint8)
    reward = rng.choice(np.array([-1.0, 0.0, 0.5, 1.0, 2.0], np.float32), size=(T, N, 2)).astype(np.float32)
    done[:, :6] = 0

    def end(t, e, r, code=1):
        done[t, e] = code
        reward[t, e] = r

    end(4, 0, (1, -1))             # env 0: ship 0 wins a game of 5 ticks,
    end(9, 0, (-1, 1))             # loses one of 5,
    end(12, 0, (1, -1))            # and wins a third of 3 after `games` is full
    end(3, 1, (0, 0), 2)           # env 1: a timeout after 4 ticks,
    end(7, 1, (1, 1))              # then a tie at reward 1: the first maximal ship
    #                                env 2: never done
    end(5, 3, (-1, 1))             # env 3: two ends on consecutive ticks (a game of one tick)
    end(6, 3, (1, -1))
    end(15, 4, (-1, -1))           # env 4: both ships lost on the last tick: no winner
    end(0, 5, (0.5, 0.75))         # env 5: a maximum below 1 on the very first tick,
    end(2, 5, (1, 2))              # then ship 1's larger reward
    return reward, done


# what the hand-written envs must give: winner, ticks, got, length, wins, finished, tick_sum
EXPECT = {
    0: ([0, 1], [5, 5], 3, 3, [2, 1], 3, 13),
    1: ([-1, 0], [4, 4], 2, 8, [1, 0], 2, 8),
    2: ([-2, -2], [0, 0], 0, 16, [0, 0], 0, 0),
    3: ([1, 0], [6, 1], 2, 9, [1, 1], 2, 7),
    4: ([-1, -2], [16, 0], 1, 0, [0, 0], 1, 16),
    5: ([-1, 1], [1, 2], 2, 13, [0, 1], 2, 3),
}


def check_expect(h):
    for e, (winner, ticks, got, length, wins, finished, tick_sum) in EXPECT.items():
        assert h['winner'][e].tolist() == winner, e
        assert h['ticks'][e].tolist() == ticks, e
        assert (int(h['got'][e]), int(h['length'][e])) == (got, length), e
        assert h['wins'][e].tolist() == wins, e
        assert (int(h['finished'][e]), int(h['tick_sum'][e])) == (finished, tick_sum), e


class Tally:
    """Counts of a sticky exploration run, as tools/gen_golden.py: gen_explore
    records them of the reference."""

    def __init__(self):
        self.out_ticks = self.entries = self.in_ticks = self.exits = self.t0_ticks = self.t0_transitions = 0
        self.hist = np.zeros(6, np.int64)

    def add(self, before, after, tick):
        """before, after: int8 [N, S] policies around one call; tick int [N]."""
        t0 = (np.asarray(tick) == 0)[:, None] & np.ones_like(before, bool)
        moved = (before < 0) != (after < 0)
        assert ((before < 0) | (after < 0) | (before == after)).all(), 'a held policy changed its control'
        self.t0_ticks += int(t0.sum())
        self.t0_transitions += int((moved & t0).sum())
        out, held = (before < 0) & ~t0, (before >= 0) & ~t0
        self.out_ticks += int(out.sum())
        self.in_ticks += int(held.sum())
        self.entries += int((moved & out).sum())
        self.exits += int((moved & held).sum())
        self.hist += np.bincount(after[moved & out].astype(np.int64), minlength=6)[:6]
