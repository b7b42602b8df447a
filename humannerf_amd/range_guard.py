"""f16-range guard of inference (the training side has autograd.OperandRangeGuard): what a ``Network`` keeps about the
status words the split-f16 MLP kernels raise in their packed weight images when a hidden activation leaves the range in
which their arithmetic is fp32-accurate.  Only ``check`` may wait for the device; ``act``, the policy, touches none."""
import collections
import warnings

import torch

from . import ops
from .config import amd_option


class ActivationRangeError(RuntimeError):
    """A hidden activation of one of the two MLPs left the range in which the split-f16 arithmetic is fp32-accurate
    (|x| >= 128, hnrf.h; the kernels clamp at 65504): the frames rendered with these weights in mlp_mode 'f16x3' are not
    the network's output."""


class InferenceRangeGuard:
    def __init__(self):
        self.hits = self.watched = self.checked = 0
        self._schedule = None       # [weights key, frames planned with it]: the audit schedule of plan
        self.reset()

    def reset(self):
        """Forget the watched frames without a verdict and the mode a hit has forced."""
        self.pending = collections.deque()      # (pinned status words [canonical, non-rigid], event behind the copy)
        self.free = []
        self.forced_mode = None                 # 'f32' after a hit with cfg.amd.on_f16_range = 'f32'

    def restart_schedule(self):
        """The next frame planned counts as the first one with its weights."""
        self._schedule = None

    def mode(self):
        return self.forced_mode or amd_option('mlp_mode', 'f16x3')

    def plan(self, mode, n_chunks, weights_key):
        """Which ray chunks of this frame run the GUARDED kernel instances (cfg.amd.f16_range_guard; the guard costs
        3 % of the frame).  'full': all.  'off': none.  'audit' (default): all chunks of the first frame after the
        weights changed (``weights_key``: the key of the packed canonical image) -- a checkpoint that does not fit the
        f16 range shows on its first frame -- then one chunk per frame, rotating, so that every region of the image and
        every pose is sampled as a sequence goes on.
        Returns (mode string for hnrf_render_frame_fwd, set of guarded chunk numbers or None = all)."""
        if mode != 'f16x3':
            return mode, None
        policy = amd_option('f16_range_guard', 'audit')
        if policy == 'full':
            return mode, None
        if policy == 'off':
            return mode + '+noguard', set()
        if self._schedule is None or self._schedule[0] != weights_key:
            self._schedule = [weights_key, 0]
        frame_no = self._schedule[1]
        self._schedule[1] += 1
        if frame_no == 0:
            return mode, None
        k = (frame_no - 1) % max(1, n_chunks)
        return mode + '+guard1:%d' % k, {k}

    def watch(self, cnl_packed, nr_packed, mode):
        """Called after a frame's inference kernels are queued: copies the two images' status words into a pinned slot
        -- behind the kernels in stream order, in front of the next frame's pack, which zeroes the non-rigid image's
        word -- and notes the event behind the copy.  Nothing waits: check looks at the slots whose copy has landed
        (Network.forward does at its start, i.e. one frame late when the host keeps up with the GPU)."""
        words = [ops.status_word(cnl_packed, 'canonical', mode),
                 None if nr_packed is None else ops.status_word(nr_packed, 'nonrigid', mode)]
        if words[0] is None and words[1] is None:
            return
        host = self.free.pop() if self.free else torch.zeros(2, dtype=torch.int32).pin_memory()
        host.zero_()
        for i, word in enumerate(words):
            if word is not None:
                host[i:i + 1].copy_(word, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.pending.append((host, ev))
        self.watched += 1

    def check(self, wait=True, upto=None):
        """Collect the status words of the watched frames whose copies have landed (``wait``: of all watched frames,
        blocking; ``upto``: block only until the first ``upto`` watched frames have their verdict).  ``checked`` counts
        the frames whose verdict is known.  Returns (canonical hit, non-rigid hit) over the frames collected; what
        follows from a hit is ``act``."""
        cnl_hit = nr_hit = 0
        while self.pending:
            host, ev = self.pending[0]
            if not ev.query():
                if not wait or (upto is not None and self.checked >= upto):
                    break
                ev.synchronize()
            self.pending.popleft()
            self.checked += 1
            cnl_hit |= int(host[0])
            nr_hit |= int(host[1])
            self.free.append(host)
        return bool(cnl_hit), bool(nr_hit)

    def act(self, cnl_hit, nr_hit):
        """The policy step (cfg.amd.on_f16_range; touches no device): False without a hit; else counts it and raises
        ActivationRangeError ('raise'), warns and forces mode 'f32' ('f32') or leaves everything as it is ('ignore'),
        returning True."""
        if not (cnl_hit or nr_hit):
            return False
        self.hits += 1
        policy = amd_option('on_f16_range', 'raise')
        msg = ("a hidden activation of the %s MLP left the range of the split-f16 arithmetic (|x| >= 128) in mlp_mode "
               "'f16x3': the frames rendered with these weights are not the network's output to fp32 accuracy; render "
               "with cfg.amd.mlp_mode = 'f32'"
               % (' and the '.join(n for n, h in (('canonical', cnl_hit), ('non-rigid', nr_hit)) if h)))
        if policy == 'ignore':
            return True
        if policy == 'f32':
            warnings.warn(msg + " -- switching this network to 'f32' (cfg.amd.on_f16_range = 'f32')")
            self.forced_mode = 'f32'
            return True
        raise ActivationRangeError(msg)
