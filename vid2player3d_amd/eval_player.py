"""Evaluating a controller: `V2PPlayer.run` (vid2player/players/v2p_player.py:133-156) for the single-player controller, as `run.py
--test` runs it over `MVAEControllerVis`.  Every step of that loop resets the envs that are done, takes the deterministic action and
steps the controller; the controller's step keeps the meters and the record (`tasks.tennis_controller.TennisControllerEval`).

`ControllerEvalPlayer(ctl, policy, reset_mode)`: ctl a `TennisControllerEval` with its generator (is_train false), target and low-level
policy attached, policy a `policies.ControllerPolicy` over it.  reset_mode 'ids' (the default) is the reference's form -
`done.nonzero()` (the host waits for the device), then `ctl.reset(ids)`; 'flags' is `ctl.reset_by_flags()` (cfg v2p `task_reset:
'device'`), the same launches every step and no host read.  Both give the same bits when `ctl._reset_root_xy` [N,2] stands in for the
generator's draw.

`run(steps)` returns `ctl.summary()`: the one host read, after the last step.  The two-player match is `match.MatchPlayer`.  Not built:
rendering, video and HTML output, the stochastic action of `is_determenistic = False`."""
import torch

RESET_MODES = ("ids", "flags")


class ControllerEvalPlayer:
    def __init__(self, ctl, policy, reset_mode="ids"):
        from .policies import ControllerPolicy
        from .tasks.tennis_controller import TennisControllerEval
        from .tasks.tennis_controller_dual import DualTennisControllerTask

        if isinstance(ctl, DualTennisControllerTask):
            raise TypeError("ControllerEvalPlayer evaluates the single-player controller; a DualTennisControllerTask is played by match.MatchPlayer")
        if not isinstance(ctl, TennisControllerEval):
            raise TypeError("ControllerEvalPlayer evaluates a TennisControllerEval (the controller with the test-mode law and the meters)")
        if not isinstance(policy, ControllerPolicy) or policy.ctl is not ctl:
            raise ValueError("ControllerEvalPlayer: policy must be a ControllerPolicy over the same controller")
        if reset_mode not in RESET_MODES:
            raise ValueError("ControllerEvalPlayer: reset_mode %r is neither 'ids' nor 'flags'" % (reset_mode,))
        self.ctl, self.policy, self.reset_mode, self.device = ctl, policy, reset_mode, ctl.device

    def _reset_done(self):
        ctl = self.ctl
        if self.reset_mode == "flags":
            ctl.reset_by_flags()
            return
        ctl.reset(ctl.reset_buf.nonzero(as_tuple=False).flatten())  # (the host read of the reference's loop)

    @torch.no_grad()
    def play(self, steps):
        """`steps` control steps of the loop, without the closing host read.  With reset_mode 'flags' nothing in it waits for the device."""
        ctl = self.ctl
        ctl.reset()  # (`env_reset()` in front of the loop: all envs once, nothing after that)
        for _ in range(int(steps)):
            self._reset_done()
            ctl.step(self.policy.act())

    def run(self, steps):
        """`steps` control steps; returns `ctl.summary()` - hit rate, forehand ratio, bounce-in rate and bounce position error over the
        envs that finished a swing, and how many did."""
        self.play(steps)
        return self.ctl.summary()
