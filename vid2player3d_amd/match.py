"""Playing a match: `V2PPlayer.run` (vid2player/players/v2p_player.py:133-156) for the two-player controller of the match configs
(`nadal_federer`, `federer_djokovic`: `dual_mode: different`, network `vid2player_dual`, two single-player checkpoints through
`dual_model_cp`).  Every step of that loop resets the pairs that are done, computes the deterministic action and steps the controller.

`MatchPlayer(ctl, policy, reset_mode)`: ctl a `DualTennisControllerTask` with its generator, target and low-level policy attached, policy
a `policies.ControllerPolicy` over it.  reset_mode 'ids' is the reference's form - `done.nonzero()` (the host waits for the device), then
`ctl.reset(ids)`; 'flags' is `ctl.reset_pairs_by_flags()`, the same launches every step and no host read.  Both give the same bits when
`ctl._reset_root_xy` [N,2] and `ctl._reset_serve_draws` [N/2,3] stand in for the draws; without them 'ids' draws from torch's stream and
'flags' from the kernels' own.

`run(steps)` keeps on the device, and returns after the run, the number of pairs that finished and the sum of `_distance` over both
players of the finished pairs - what the reference ranks matches by (mvae_controller_vis_dual.py:167).  Rendering and recording are not
built."""
import torch

RESET_MODES = ("ids", "flags")


class MatchPlayer:
    def __init__(self, ctl, policy, reset_mode="ids"):
        from .policies import ControllerPolicy
        from .tasks.tennis_controller_dual import DualTennisControllerTask

        if not isinstance(ctl, DualTennisControllerTask):
            raise TypeError("MatchPlayer plays a DualTennisControllerTask (a match has two players)")
        if not isinstance(policy, ControllerPolicy) or policy.ctl is not ctl:
            raise ValueError("MatchPlayer: policy must be a ControllerPolicy over the same controller")
        if reset_mode not in RESET_MODES:
            raise ValueError("MatchPlayer: reset_mode %r is neither 'ids' nor 'flags'" % (reset_mode,))
        self.ctl, self.policy, self.reset_mode, self.device = ctl, policy, reset_mode, ctl.device
        self.finished_pairs = torch.zeros((), dtype=torch.int64, device=self.device)
        self.finished_distance = torch.zeros((), dtype=torch.float64, device=self.device)

    def _reset_done(self):
        ctl = self.ctl
        if self.reset_mode == "flags":
            ctl.reset_pairs_by_flags()
            return
        ids = ctl.reset_buf.nonzero(as_tuple=False).flatten()  # (the host read of the reference's loop)
        xy, draws = ctl._reset_root_xy, ctl._reset_serve_draws
        ctl.reset(ids, root_xy=None if xy is None or ids.numel() == 0 else xy[ids], serve_vel_draws=None if draws is None or ids.numel() == 0 else draws[ids[::2] >> 1])

    def _count_finished(self):
        """(the dual step's law raises both flags of a pair; either one counts, as in `reset_pairs_by_flags`)"""
        ctl = self.ctl
        done = (ctl.reset_buf.view(-1, 2) != 0).any(1)
        self.finished_pairs += done.sum()
        self.finished_distance += (ctl._distance.view(-1, 2).sum(1).double() * done).sum()

    @torch.no_grad()
    def play(self, steps):
        """The loop of `run` without its closing host read: returns the two device scalars (`finished_pairs` int64, `finished_distance`
        float64) of this run.  With reset_mode 'flags' nothing in it waits for the device."""
        ctl = self.ctl
        ctl.reset()
        self.finished_pairs.zero_()
        self.finished_distance.zero_()
        for _ in range(int(steps)):
            self._reset_done()
            ctl.step(self.policy.act())
            self._count_finished()
        return self.finished_pairs, self.finished_distance

    def run(self, steps):
        """`steps` control steps; returns (finished pairs, the summed distance of the finished pairs) of this run as Python numbers - the
        one host read, after the last step."""
        pairs, distance = self.play(steps)
        return int(pairs), float(distance)
