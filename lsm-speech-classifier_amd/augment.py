"""The augmentation recipe in one place: the per-clip plans of a step (`StepPlans`) and the device stages that act on them
in the recipe's order (`AugmentChain`): speed (SPEC.md §1.12), reverberation (§1.11), mixer (§1.10), and the mask inside the
spike encoder behind all three (§1.13).  `pipeline.HotPath` and the drop-in scripts drive the stages through here."""
from __future__ import annotations

from typing import NamedTuple

from .frontend import indexed_device


class StepPlans(NamedTuple):
    """The per-clip plans of one batch, one shard or a whole listing: a `frontend.SpeedPlan`, `ReverbPlan`, `MixPlan` and
    `MaskPlan`, each None where the clips are left alone."""
    speed: object = None
    reverb: object = None
    mix: object = None
    mask: object = None

    def part(self, lo: int, hi: int) -> "StepPlans":
        """The plans of clips ``lo .. hi - 1``: a batch's or a shard's slice."""
        return StepPlans(*(None if p is None else p.part(lo, hi) for p in self))

    def take(self, idx) -> "StepPlans":
        """The plans of the clips ``idx`` names, in that order (a split of the listing)."""
        return StepPlans(*(None if p is None else p.take(idx) for p in self))

    def check_covers(self, n: int) -> None:
        """Every plan holds one entry per clip of ``n`` clips, or ValueError."""
        if self.mask is not None and not (len(self.mask.freq) == len(self.mask.time) == n):
            raise ValueError(f"the mask plan covers {len(self.mask.freq)} / {len(self.mask.time)} clips, audio has {n}")
        if self.speed is not None and len(self.speed.choice) != n:
            raise ValueError(f"the speed plan covers {len(self.speed.choice)} clips, audio has {n}")
        if self.reverb is not None and len(self.reverb.rows) != n:
            raise ValueError(f"the reverb plan covers {len(self.reverb.rows)} clips, audio has {n}")
        if self.mix is not None and len(self.mix.rows) != n:
            raise ValueError(f"the plan covers {len(self.mix.rows)} clips, audio has {n}")

    def mask_keyword(self) -> dict:
        """What `SpikeFrontEnd.encode` / `pipeline.step_fused` get beside the audio: ``mask=`` only when there is a mask, so
        that a step without one is launched as it always was."""
        return {} if self.mask is None else {"mask": self.mask}


class AugmentChain:
    """The device stages in front of the front end, each a stage or None: `frontend.SpeedPerturber`, `Reverberator`,
    `NoiseMixer`."""

    def __init__(self, speed=None, reverb=None, mixer=None):
        self.speed, self.reverb, self.mixer = speed, reverb, mixer

    def check_device(self, device) -> None:
        """Every stage lives on the front end's ``device``, or ValueError."""
        for name, stage in (("mixer", self.mixer), ("reverberator", self.reverb), ("speed perturber", self.speed)):
            if stage is not None and indexed_device(stage.device) != indexed_device(device):
                raise ValueError(f"{name} on {stage.device}, front end on {device}")

    def refuse(self, plans: StepPlans, front_end: bool = True) -> None:
        """A plan needs its stage and a step that has a front end, or ValueError."""
        for key, plan, stage, name in (("mix", plans.mix, self.mixer, "a mixer"),
                                       ("reverb", plans.reverb, self.reverb, "a reverberator"),
                                       ("speed", plans.speed, self.speed, "a speed perturber")):
            if plan is not None and (stage is None or not front_end):
                raise ValueError(f"submit({key}=...) needs a HotPath built with {name} and a step that has a front end")

    def apply(self, x, plans: StepPlans, buffer=None):
        """``x`` (B, n_samples) through the stages whose plan is not None, on the current stream: speed, then reverberation,
        then mixer; a stage without a plan launches nothing.  ``buffer``: a callable ``(stage name, shape) -> tensor`` that
        hands out the stage's output buffer ("speed", "reverb", "mix"); None: the stage allocates."""
        self.refuse(plans)

        def out(name):
            return None if buffer is None else buffer(name, tuple(x.shape))

        if plans.speed is not None:
            x = self.speed.perturb(x, plans.speed.choice, out=out("speed"))
        if plans.reverb is not None:
            x = self.reverb.reverb(x, plans.reverb.rows, out=out("reverb"))
        if plans.mix is not None:
            m = plans.mix
            x = self.mixer.mix(x, m.snr_db, m.rows, m.offsets, m.shift, m.scale, out=out("mix"))
        return x

    def speed_ragged(self, x, lengths, plans: StepPlans, time_bins: int | None = None, out=None):
        """The recipe's first stage on a ragged batch (SPEC.md §1.18), ahead of `apply_ragged`: ``x`` (B, n_samples) rows
        at one stride, clip b their first ``lengths[b]`` samples, played at the speeds of ``plans.speed`` -> ``(x, samples,
        bins)`` as `frontend.SpeedPerturber.perturb_ragged` returns them: rows of the same stride, every clip at its new
        length with +0.0 behind, and the new lengths in samples and in time bins as int32 device tensors (``time_bins``:
        the bins of a row, n_samples // 160 by default; ``out``: a caller-owned output buffer of ``x``'s shape).  A stage
        of its own because it changes the lengths that every later stage takes; `apply_ragged` then runs with ``plans``
        less its speed plan.  Without a speed plan nothing is launched and ``(x, None, None)`` comes back."""
        self.refuse(plans)
        if plans.speed is None:
            return x, None, None
        return self.speed.perturb_ragged(x, lengths, plans.speed.choice, time_bins=time_bins, out=out)

    def apply_ragged(self, x, lengths, plans: StepPlans):
        """`apply` for a ragged batch (SPEC.md §1.16): ``x`` (B, n_samples) rows at one stride, clip b their first
        ``lengths[b]`` samples.  Reverberation runs at the row stride -- it is causal, so a clip's own samples are those of
        the clip alone, and its tail behind the clip is ignored by what follows -- then the ragged mixer takes every clip at
        its own length.  Speed perturbation changes a clip's length and is not offered here: it is `speed_ragged`, ahead of
        this call.  Without a plan nothing is launched and ``x`` comes back as it is."""
        self.refuse(plans)
        if plans.speed is not None:
            raise ValueError("speed perturbation is not offered on ragged batches: a speed factor changes a clip's bin count")
        if plans.reverb is not None:
            x = self.reverb.reverb(x, plans.reverb.rows)
        if plans.mix is not None:
            m = plans.mix
            x = self.mixer.mix_ragged(x, lengths, m.snr_db, m.rows, m.offsets, m.shift, m.scale)
        return x
