"""Validation metrics of a training run, per epoch (the reference's common/utils/metric_history.py: same methods, same answers).

    hist = MetricHistory()
    hist.add_metric("MPJPE", higher_is_better=False)
    hist.add_data("MPJPE", value=52.1, step=epoch)
    value, epoch = hist.best_value("MPJPE")          # the FIRST best entry on ties, (None, None) while empty

``state_dict()`` / ``from_state_dict()`` carry it through a training checkpoint (run_train's exact resume).
"""
import numpy as np


class MetricHistory(object):

    def __init__(self):
        self.metrics = []
        self.higher = []
        self.history = {}

    def add_metric(self, metric, higher_is_better=True):
        if metric in self.metrics:
            raise AssertionError(f"metric {metric} is already tracked")
        self.metrics.append(metric)
        self.higher.append(higher_is_better)
        self.history[metric] = []

    def add_data(self, metric, value, step):
        self.history[metric].append((step, value))

    def best_value(self, metric):
        """-> (best value, its step)."""
        entries = self.history[metric]
        if not entries:
            return None, None
        values = np.array([v for _, v in entries], np.float64)
        at = int(np.argmax(values) if self.higher[self.metrics.index(metric)] else np.argmin(values))
        step, value = entries[at]
        return value, step

    def value_at_step(self, metric, step):
        for s, v in self.history[metric]:
            if s == step:
                return v
        return None

    def latest_value(self, metric):
        entries = self.history[metric]
        if not entries:
            return None
        return max(entries, key=lambda e: e[0])[1]

    def _line(self, metric, value, step):
        return f"{metric}: {value} (step {step})" if "loss" in metric else f"{metric}: {value:.3f} (step {step})"

    def print_best(self, log=print):
        for metric in self.metrics:
            value, step = self.best_value(metric)
            log(self._line(metric, value, step))

    def print_all_for_best_metric(self, metric, log=print):
        _, step = self.best_value(metric)
        for m in self.metrics:
            log(self._line(m, self.value_at_step(m, step), step))

    def state_dict(self):
        return {"metrics": list(self.metrics), "higher": [bool(h) for h in self.higher],
                "history": {m: [[int(s), float(v)] for s, v in self.history[m]] for m in self.metrics}}

    @classmethod
    def from_state_dict(cls, sd):
        h = cls()
        for m, hi in zip(sd["metrics"], sd["higher"]):
            h.add_metric(m, higher_is_better=hi)
            h.history[m] = [(int(s), float(v)) for s, v in sd["history"][m]]
        return h
