"""The binned metrics, the cluster table and the clustering scores of a collated batch on the CPU wave64 emulator (the real
kernel sources of csrc/tracking_metrics.hip and csrc/cluster_scores.hip): every case of tests/oc_details_batch_cases.py
against the single-event oracles applied per event, and the host-side argument checks of the three batched C entries."""

import contextlib

import pytest
import torch

import oc_details_batch_cases as C
from emul_util import emulated, emulator_lib

pytestmark = pytest.mark.emul
DEVICE = "cpu"


@contextlib.contextmanager
def emulated_cpu():
    """the emulator takes host pointers: the package must not move its inputs to a GPU that happens to be there"""
    old = torch.cuda.is_available
    torch.cuda.is_available = lambda: False
    try:
        with emulated():
            yield
    finally:
        torch.cuda.is_available = old


@pytest.mark.parametrize("sizes", (C.EVENTS, C.INNER_EVENTS))
def test_windows_and_table_per_event(sizes):
    with emulated_cpu():
        C.case_windows_and_table(DEVICE, sizes)


def test_majority_tie_inside_the_event():
    with emulated_cpu():
        C.case_tie(DEVICE)


def test_label_beyond_its_event_is_refused():
    with emulated_cpu():
        C.case_bad_label(DEVICE)


def test_spectra_and_scores_per_event():
    with emulated_cpu():
        C.case_spectra(DEVICE)


def test_spectra_capacity_bounds_every_split():
    C.case_capacity(emulator_lib())


def test_one_event_is_todays_call():
    with emulated_cpu():
        C.case_one_event(DEVICE)


def test_performance_details_and_binned_metrics_on_a_collated_batch():
    with emulated_cpu():
        C.case_scanner(DEVICE)


def test_batched_entries_validate_on_the_host():
    C.case_host_validation(emulator_lib())
