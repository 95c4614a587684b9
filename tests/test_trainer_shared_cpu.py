"""What the trainers share in trainer/baseTrainer.py and no GPU is needed for: the loader cycler (``LoaderCycle``) and the command
line (``make_parser`` / ``run_main``) of the seven trainer modules that have a ``main``."""
import importlib

import pytest

import smsut_amd  # noqa: F401
from smsut_amd.trainer import baseTrainer as B


class RecordingLoader:
    """Yields ``batches`` once per ``iter()``; ``entered`` counts how often ``__iter__`` was entered."""

    def __init__(self, batches):
        self.batches, self.entered = list(batches), 0

    def __iter__(self):
        self.entered += 1
        return iter(self.batches)


def test_cycler_restarts_an_exhausted_loader():
    ld = RecordingLoader(["a", "b"])
    cyc = B.LoaderCycle(ld)
    assert [next(cyc) for _ in range(5)] == ["a", "b", "a", "b", "a"]
    assert ld.entered == 3


def test_cycler_calls_iter_on_construction_in_the_order_it_is_built():
    order = []

    class Loader(RecordingLoader):
        def __iter__(self):
            order.append(self.batches[0])
            return super().__iter__()

    lb, ul = Loader(["lb"]), Loader(["ul"])
    c_lb, c_ul = B.LoaderCycle(lb), B.LoaderCycle(ul)
    assert order == ["lb", "ul"] and (lb.entered, ul.entered) == (1, 1)      # before any next()
    assert next(c_ul) == "ul" and next(c_lb) == "lb"
    assert order == ["lb", "ul"]                                              # the first next() uses the iterator made above


def test_cycler_raises_on_a_loader_that_yields_nothing():
    with pytest.raises(RuntimeError):
        next(B.LoaderCycle(RecordingLoader([])))
    ld = RecordingLoader(["a"])
    cyc = B.LoaderCycle(ld)
    assert next(cyc) == "a"
    ld.batches = []                                                           # runs dry later: one fresh pass, then the error
    with pytest.raises(RuntimeError):
        next(cyc)
    assert ld.entered == 2


MODULES = (("unetTrainer", "UnetTrainer", ("train", "test")), ("crossPseTrainer", "crossPseTrainer", ("train", "test")),
           ("meanTeacherTrainer", "meanTeacherTrainer", ("train", "test")), ("dtcTrainer", "dtcTrainer", ("train", "test")),
           ("uganTrainer", "UGANTrainer", ("train", "test")), ("uganConsisTrainer", "UGANConsisTrainer", ("train", "test", "pseudo")),
           ("coraNetTrainer", "coraNetTrainer", ("pretrain", "train", "test", "pseudo")))
# what each phase does after the trainer is built: (phase the trainer is built with, the calls that follow)
FLOW = {"train": ("train", [("fit", "inTurn")]),
        "pretrain": ("train", [("prefit", "inTurn")]),
        "test": ("test", [("load_model", "007", "last"), ("test", "inTurn", "ROOT/007")]),
        "pseudo": ("pseudo", [("load_model", "007", "last"), ("PSEUDO", "inTurn", "ROOT/007")])}
PSEUDO = {"UGANConsisTrainer": "saving_pseudo", "coraNetTrainer": "save_pseudo"}


@pytest.mark.parametrize("module,klass,phases", MODULES, ids=[m[0] for m in MODULES])
def test_main_takes_exactly_its_phases_and_runs_the_common_flow(monkeypatch, module, klass, phases):
    mod = importlib.import_module("smsut_amd.trainer." + module)
    calls = []

    class Fake:
        expr_root = "ROOT"

        def __init__(self, phase, args):
            calls.append(("init", phase, args))

        def __getattr__(self, name):
            return lambda *a: calls.append((name,) + a)

    monkeypatch.setattr(mod, klass, Fake)
    monkeypatch.setattr(B, "seed_all", lambda seed=None: calls.append(("seed",)))
    for phase in phases:
        del calls[:]
        mod.main(["-p", phase, "-i", "007"])
        built_as, then = FLOW[phase]
        then = [tuple(PSEUDO[klass] if v == "PSEUDO" else v for v in c) for c in then]
        assert calls[0] == ("seed",) and calls[1][:2] == ("init", built_as) and calls[2:] == then, (phase, calls)
        args = calls[1][2]
        assert (args.phase, args.fold, args.expr_name, args.model_id, args.which_ckpt) == (phase, 0, None, "007", "last")
    for other in {"pretrain", "train", "test", "pseudo", "nonsense"} - set(phases):
        del calls[:]
        with pytest.raises(SystemExit):
            mod.main(["-p", other])
        assert calls == []
    del calls[:]
    mod.main(["-p", "test", "-f", "3", "-nm", "x", "-i", "000", "-wh", "best"])
    args = calls[1][2]
    assert (args.fold, args.expr_name, args.model_id, args.which_ckpt) == (3, "x", "000", "best")


def test_make_parser_defaults_and_choices():
    p = B.make_parser(("train", "test"))
    args = p.parse_args([])
    assert (args.phase, args.fold, args.expr_name, args.model_id, args.which_ckpt) == (None, 0, None, None, "last")
    assert {a.dest: a.choices for a in p._actions}["phase"] == ("train", "test")
    from smsut_amd.trainer import coraNetTrainer
    cora = coraNetTrainer.make_parser()
    assert {a.dest: a.choices for a in cora._actions}["phase"] == ("pretrain", "train", "test", "pseudo")
    assert cora.parse_args([]).which_ckpt == "last" and cora.parse_args([]).fold == 0
