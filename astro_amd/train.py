"""The reference trainer's loop (astro/rl.py: QBotTrainer.__call__ / reward /
_step, rl.py:249-328, and train, rl.py:335-374) for a whole ``BatchedEnv``, from
the device pieces: ``env.features`` and ``env.qcontrols`` (astro_qnet.h) with
``actor.EpsilonGreedy`` (astro_actor.h), ``env.step``, ``ReplayBuffer``
(astro_replay.h) and ``QNetwork.sgd_step`` (astro_qtrain.h).

One ``QTrainer.tick()`` is one tick of every env and, once the ring holds
``n_samples`` eligible experiences, ``n_ministeps`` optimisation steps -- the
reference takes them when an n-step window closes, every ``n_steps`` ticks per
bot; with thousands of envs a window closes somewhere on every tick.

Options, all off by default: an ``astro_amd.optim`` update rule instead of
``sgd_step``, a frozen target network for the targets, Double-DQN targets
(astro_qopt.h), and an opponent as ship 1: a scripted bot, a fixed network or a
snapshot of the learner refreshed every K steps (astro_qduel.h).

``Distiller`` is the other way to train the same network: no replay and no
bootstrap, the targets are a ``fork.Lookahead``'s search values for all six
controls of every state (astro_search.h).
"""
import torch

from . import actor


class QTrainer:
    """env: the training ``BatchedEnv``; net: a ``qnet.QNetwork``; buf: a
    ``ReplayBuffer`` of the env's shape; explore: an ``actor.EpsilonGreedy`` of
    the env (or None: greedy).  ``seed`` keys the replay sampling; the
    exploration has its own.

    optimizer: an ``astro_amd.optim`` rule (``net.step`` instead of
    ``net.sgd_step(..., lr=lr)``; ``lr`` is then the optimizer's own).
    target_sync (needs an optimizer): the targets come from ``self.target``, a
    frozen ``net.clone()`` -- an int K: hard-copied every K optimisation steps;
    a float in (0, 1): Polyak-averaged with that tau on every step; both inside
    the optimiser's launch.  double: Double-DQN targets (the action the online
    network prefers, valued by the target network).  opponent: 'script',
    'nothing' or 'random' -- ship 1 plays ``env.controls(opponent, seed, t)``
    instead of the network's choice (its experiences still go to the ring:
    Q-learning is off-policy; its exploration state still advances), and ship
    1's Q values are not computed at all.  opponent=<QNetwork>: ship 1 plays
    that fixed network, ``self.rival``, in the same launch that evaluates
    ``net`` for ship 0.  opponent='snapshot' with opponent_sync=K (an int >= 1;
    required with 'snapshot', rejected otherwise): ``self.rival`` is a
    ``net.clone()``, refreshed with ``rival.copy_from(net)`` after every K-th
    optimisation step -- self-play against a frozen copy of oneself.  With a
    network as ship 1 ``explore`` applies to both ships, and both ships'
    experiences go to the ring as before.  opponent='pool' with pool_size=K
    (1..31) and opponent_sync=J: ``self.rivals`` is K clones of ``net``, ship 1
    of the j-th of K blocks of envs plays ``rivals[j]`` (``league.Pool.versus``,
    astro_qpool.h: still one acting launch per tick), and after every J-th
    optimisation step the oldest slot is refreshed with ``copy_from(net)``,
    round robin from slot 0 -- self-play against copies of oneself of K
    different ages.  pool_size=1 is 'snapshot' bit for bit.  pool_size goes with
    'pool' only.  opponent=<league.Script>: ship 1 plays a ScriptBot with those
    arguments.  opponent=<list or tuple> of ``QNetwork``s, ``Script``s and bot
    names: a fixed ladder, ``self.ladder`` -- ship 1 of the j-th of K blocks of
    envs plays ``opponent[j]`` (``league.Seats.versus``: the networks' launch,
    the exploration, then one astro_controls_seats launch, astro_seats.h;
    exploration never alters a scripted seat's control).  ``['script']`` acts as
    'script' does, bit for bit."""

    def __init__(self, env, net, buf, explore, n_samples=1024, n_ministeps=1, lr=1e-2, seed=0,
                 optimizer=None, target_sync=None, double=False, opponent=None, opponent_sync=None, pool_size=None):
        if buf.n_env != env.n_env or buf.nships != env.S:
            raise ValueError('the replay buffer is [%d envs, %d ships], the env [%d, %d]'
                             % (buf.n_env, buf.nships, env.n_env, env.S))
        self.env, self.net, self.buf, self.explore = env, net, buf, explore
        self.n_samples, self.n_ministeps, self.lr, self.seed = int(n_samples), int(n_ministeps), float(lr), int(seed)
        self.nstep = 0     # optimisation steps so far (rl.QNetworkTrainer.nstep)
        self.last = None
        self.optimizer, self.double, self.opponent = optimizer, bool(double), opponent
        self.target, self.sync_every, self.tau = None, None, 1.0
        if target_sync is not None:
            if optimizer is None:
                raise ValueError('target_sync needs an optimizer (the target follows inside its launch)')
            if isinstance(target_sync, int) and not isinstance(target_sync, bool) and target_sync >= 1:
                self.sync_every = target_sync
            elif isinstance(target_sync, float) and 0.0 < target_sync < 1.0:
                self.tau = target_sync
            else:
                raise ValueError('target_sync must be an int >= 1 (steps between hard copies) or a float in (0, 1)')
            self.target = net.clone()
        self.rival, self.rival_every, self.rivals, self.ladder = None, None, None, None
        from .league import Script, Seats
        if isinstance(opponent, (Script, list, tuple)):   # one scripted rival with its own arguments, or a fixed ladder
            if pool_size is not None:
                raise ValueError("pool_size goes with opponent='pool' only")
            if opponent_sync is not None:
                raise ValueError("opponent_sync goes with opponent='snapshot' or 'pool' only")
            if env.S != 2:
                raise ValueError('opponent needs a two-ship env')
            self.ladder = (opponent,) if isinstance(opponent, Script) else tuple(opponent)
            self._acting, self._bot = Seats.versus(env, net, self.ladder), None
            return
        pool = isinstance(opponent, str) and opponent == 'pool'
        if pool_size is not None and not pool:
            raise ValueError("pool_size goes with opponent='pool' only")
        if pool or (isinstance(opponent, str) and opponent == 'snapshot'):
            if not (isinstance(opponent_sync, int) and not isinstance(opponent_sync, bool) and opponent_sync >= 1):
                raise ValueError('opponent=%r needs opponent_sync, an int >= 1 (optimisation steps '
                                 'between refreshes)' % opponent)
            if pool and not (isinstance(pool_size, int) and not isinstance(pool_size, bool) and 1 <= pool_size <= 31):
                raise ValueError("opponent='pool' needs pool_size, an int in [1, 31]")
            if env.S != 2:
                raise ValueError('opponent needs a two-ship env')
            self.rival_every = opponent_sync
            if pool:
                self.rivals = [net.clone() for _ in range(pool_size)]
            else:
                self.rival = net.clone()
        else:
            if opponent_sync is not None:
                raise ValueError("opponent_sync goes with opponent='snapshot' or 'pool' only")
            env._check_opponent(opponent)
            if opponent is not None and not isinstance(opponent, str):
                self.rival = opponent
        # what env.qcontrols takes, and the scripted name whose controls fill ship 1's column
        if pool:
            from .league import Pool
            self._acting, self._bot = Pool.versus(env, net, self.rivals), None
        else:
            self._acting, self._bot = env._with_opponent(net, opponent if self.rival is None else self.rival)

    def _targets(self, r, d, nf, term):
        valuer = self.net if self.target is None else self.target
        return valuer.td_targets(r, d, nf, term, online=self.net) if self.double else valuer.td_targets(r, d, nf, term)

    def _step(self, f, a, targets):
        if self.optimizer is None:
            return self.net.sgd_step(f, a, targets, lr=self.lr)
        follow = self.target
        if self.sync_every is not None and (self.nstep + 1) % self.sync_every != 0:
            follow = None
        return self.net.step(f, a, targets, self.optimizer, target_net=follow, tau=self.tau)

    def tick(self):
        """One tick of acting and (when the ring is ready) training.  Returns
        ``dict(loss=..., n=...)`` like rl.QBotTrainer._step (the summed loss
        of the last ministep as a device scalar, the number of samples as a
        device int32 scalar), or None while the ring fills.  No host
        synchronisation."""
        env, net, buf = self.env, self.net, self.buf
        t = buf.t
        env.features(out=buf.head())
        control = env.qcontrols(self._acting, seed=self.seed, tick0=t, explore=self.explore)   # (seed: a Seats' 'random')
        if self._bot is not None:
            control[:, 1] = env.controls(self._bot, self.seed, t)[:, 1]
        _, reward, done = env.step(control)
        buf.push(control, reward, done)
        if buf.eligible_lower_bound() < self.n_samples:
            return None
        out = None
        for m in range(self.n_ministeps):
            ids = buf.sample(self.n_samples, seed=self.seed, draw=t * self.n_ministeps + m)
            f, a, r, d, nf, term = buf.gather(ids)
            loss = self._step(f, a, self._targets(r, d, nf, term))
            buf.update_loss(ids, loss)
            self.nstep += 1
            if self.rival_every is not None and self.nstep % self.rival_every == 0:
                if self.rivals is None:
                    self.rival.copy_from(net)
                else:   # the oldest slot: round robin from slot 0
                    self.rivals[(self.nstep // self.rival_every - 1) % len(self.rivals)].copy_from(net)
            out = dict(loss=loss.sum(), n=torch.full((), ids.shape[0], dtype=torch.int32, device=loss.device))
        self.last = out
        return out

    def run(self, ticks):
        """``ticks`` calls of ``tick``; returns the last result (or None)."""
        out = None
        for _ in range(int(ticks)):
            out = self.tick()
        return out

    def validate(self, eval_env, games=1, opponent=None, record=None):
        """rl.train's validation (rl.py:352-369): ``eval_env.play_q(net,
        opponent, games)`` with the greedy network from the env's current
        states, as ``actor.Episodes.summary()`` -- the share of games won by
        each ship (ship 0 is the network), the share without a winner and the
        median length in ticks.  opponent: None, a scripted bot's name or a
        ``QNetwork`` (``self.rival``, say) as ship 1.  record: a
        ``record.Recorder`` of ``eval_env`` (see ``play_q``): the games of its
        envs, with the network's Q values, as rl.train saves its validation
        game (rl.py:354-355).  Synchronises."""
        return eval_env._play_q(self.net, opponent, games, None, None, 0, record).summary()


class Distiller:
    """Train a Q-network on a search's values: ``teacher`` (a
    ``fork.Lookahead`` of ``env`` for ship 0) plays ship 0 and, on every tick,
    its ``values()`` -- one number for EACH of the six controls of every env --
    are the regression targets of all six outputs of ``net``.  Nothing
    bootstraps: a target is the search's own estimate.

    One ``tick()``: ``f = env.features()``; ``v = teacher.values()``; ship 0
    plays ``teacher.controls(values=v)`` (then ``explore.apply``, an
    ``actor.EpsilonGreedy`` of ``env``, if given); the other ship plays
    ``env.controls(opponent)`` ('script', 'nothing' or 'random'; its control is
    final); ``env.step``; then ONE training step through ``net.step`` (with an
    ``astro_amd.optim`` optimizer) or ``net.sgd_step(lr=lr)`` on 6 n samples --
    every chosen env's features six times, with the actions 0..5 and the
    targets ``v``'s row.  Six targets per state are six samples to the existing
    gradient kernel.  envs_per_step: n, the envs trained on per tick (default
    all): tick t takes the n entries from position ``t * n`` (cyclically) of a
    permutation of the envs that is drawn once from ``seed``.

    leaf_sync=J > 0: expert iteration -- ``teacher.leaf`` is kept a
    ``net.clone()`` (set here, replacing what the teacher had), hard-copied
    from ``net`` after every J-th step; the teacher then values unended
    branches with the student.  J = 0 leaves the teacher as it is."""

    def __init__(self, env, net, teacher, optimizer=None, lr=1e-2, opponent='script', explore=None, envs_per_step=None,
                 leaf_sync=0, seed=0):
        from .fork import Lookahead
        from .qnet import QNetwork
        if not isinstance(teacher, Lookahead) or teacher.env is not env:
            raise ValueError('teacher must be a fork.Lookahead of this env')
        if teacher.ship != 0:
            raise ValueError('teacher must play ship 0, not ship %d' % teacher.ship)
        if not isinstance(net, QNetwork) or net.nships != env.S or net.nout != Lookahead.NCONTROL:
            raise ValueError('net must be a QNetwork for %d ships with %d outputs' % (env.S, Lookahead.NCONTROL))
        if env.S > 1 and opponent not in ('script', 'nothing', 'random'):
            raise ValueError("opponent must be 'script', 'nothing' or 'random', got %r" % (opponent,))
        if explore is not None and getattr(explore, 'env', None) is not env:
            raise ValueError('explore belongs to another env')
        n = env.n_env if envs_per_step is None else envs_per_step
        if not (isinstance(n, int) and not isinstance(n, bool) and 1 <= n <= env.n_env):
            raise ValueError('envs_per_step must be an int in [1, %d], got %r' % (env.n_env, envs_per_step))
        if not (isinstance(leaf_sync, int) and not isinstance(leaf_sync, bool) and leaf_sync >= 0):
            raise ValueError('leaf_sync must be an int >= 0 (steps between hard copies; 0: off), got %r' % (leaf_sync,))
        self.env, self.net, self.teacher, self.optimizer = env, net, teacher, optimizer
        self.lr, self.opponent, self.explore, self.seed = float(lr), opponent, explore, int(seed)
        self.envs_per_step, self.leaf_sync = n, leaf_sync
        self.nstep = 0          # ticks, which are optimisation steps, so far
        self.last = None
        A = Lookahead.NCONTROL
        self._action = (torch.arange(n * A, device=env.device) % A).to(torch.int8)
        self._order = None
        if n < env.n_env:
            g = torch.Generator().manual_seed(self.seed)
            self._order = torch.randperm(env.n_env, generator=g).to(env.device)
            self._window = torch.arange(n, device=env.device)
        if leaf_sync:
            teacher.leaf = net.clone()

    def tick(self):
        """One tick of acting and one training step.  Returns the mean loss as
        a device scalar; no host synchronisation."""
        env, net, teacher, t = self.env, self.net, self.teacher, self.nstep
        f = env.features()
        v = teacher.values()
        c = torch.empty((env.n_env, env.S), dtype=torch.int8, device=env.device)
        c[:, 0] = teacher.controls(values=v)
        if self.explore is not None:
            self.explore.apply(c, t)
        if env.S > 1:       # (after the exploration: the other ship's control is final)
            c[:, 1] = env.controls(self.opponent, self.seed, t)[:, 1]
        env.step(c)
        if self._order is not None:
            ids = self._order[(self._window + t * self.envs_per_step) % env.n_env]
            f, v = f[ids], v[ids]
        f6 = f.repeat_interleave(v.shape[1], 0)
        target = v.reshape(-1)
        if self.optimizer is None:
            loss = net.sgd_step(f6, self._action, target, lr=self.lr)
        else:
            loss = net.step(f6, self._action, target, self.optimizer)
        self.nstep += 1
        if self.leaf_sync and self.nstep % self.leaf_sync == 0:
            teacher.leaf.copy_from(net)
        self.last = loss.mean()
        return self.last

    def run(self, ticks):
        """``ticks`` calls of ``tick``; returns the last mean loss (or None)."""
        out = None
        for _ in range(int(ticks)):
            out = self.tick()
        return out

    def validate(self, eval_env, games=1, opponent=None, record=None):
        """``QTrainer.validate``'s: the NETWORK plays greedily, without search
        -- ``eval_env.play_q(net, opponent, games)`` as
        ``actor.Episodes.summary()``.  Synchronises."""
        return eval_env._play_q(self.net, opponent, games, None, None, 0, record).summary()
