"""Learning-rate schedules with the formulas of tf.keras.optimizers.schedules. A schedule is a callable `schedule(step)`
evaluated on the HOST once per step (step = the optimizer's `iterations` before the increment: 0 at the first step); the
value reaches the kernels through the optimizer's device scalars, so a recorded step follows it too."""
import math


class LearningRateSchedule:
    def __call__(self, step):
        raise NotImplementedError

    def get_config(self):
        return {k: v for k, v in vars(self).items() if not k.startswith("_")}


class ExponentialDecay(LearningRateSchedule):
    """initial_learning_rate * decay_rate ** (step / decay_steps); staircase: the exponent is floored"""

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False, name=None):
        if decay_steps <= 0:
            raise ValueError("decay_steps must be positive")
        self.initial_learning_rate = float(initial_learning_rate)
        self.decay_steps, self.decay_rate = decay_steps, float(decay_rate)
        self.staircase, self.name = bool(staircase), name

    def __call__(self, step):
        p = step / self.decay_steps
        if self.staircase:
            p = math.floor(p)
        return self.initial_learning_rate * self.decay_rate ** p


class PiecewiseConstantDecay(LearningRateSchedule):
    """values[0] while step <= boundaries[0], values[i] for boundaries[i-1] < step <= boundaries[i], values[-1] beyond"""

    def __init__(self, boundaries, values, name=None):
        if len(values) != len(boundaries) + 1:
            raise ValueError("PiecewiseConstantDecay needs exactly one more value than boundaries")
        if any(b <= a for a, b in zip(boundaries, boundaries[1:])):
            raise ValueError("boundaries must be strictly increasing")
        self.boundaries, self.values, self.name = list(boundaries), [float(v) for v in values], name

    def __call__(self, step):
        for b, v in zip(self.boundaries, self.values):
            if step <= b:
                return v
        return self.values[-1]


class CosineDecay(LearningRateSchedule):
    """initial_learning_rate * ((1 - alpha) * 0.5 * (1 + cos(pi * min(step, decay_steps) / decay_steps)) + alpha)"""

    def __init__(self, initial_learning_rate, decay_steps, alpha=0.0, name=None):
        if decay_steps <= 0:
            raise ValueError("decay_steps must be positive")
        self.initial_learning_rate = float(initial_learning_rate)
        self.decay_steps, self.alpha, self.name = decay_steps, float(alpha), name

    def __call__(self, step):
        s = min(step, self.decay_steps)
        cosine = 0.5 * (1.0 + math.cos(math.pi * s / self.decay_steps))
        return self.initial_learning_rate * ((1.0 - self.alpha) * cosine + self.alpha)
