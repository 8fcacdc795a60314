"""Minimal stand-in for third-party torchmetrics (absent here), for tools/gen_golden_val.py: the reference's metric classes
(src/modules/utils.py:335-541) need a base class with `add_state` and nothing else; MetricCollection is only a name that
src/modules/raft_spline.py imports."""


class Metric:
    def __init__(self, **kwargs):
        pass

    def add_state(self, name, default, dist_reduce_fx=None):
        setattr(self, name, default.clone())


class MetricCollection:
    pass
