"""The binned metrics, the cluster table and the clustering scores of a collated batch on the GPU: every case of
tests/oc_details_batch_cases.py against the single-event oracles applied per event (exact: counts, table rows, spectra
and the floats the host derives from them)."""

import pytest

import oc_details_batch_cases as C

pytestmark = pytest.mark.gpu
DEVICE = "cuda"


@pytest.mark.parametrize("sizes", (C.EVENTS, C.INNER_EVENTS))
def test_windows_and_table_per_event(sizes):
    C.case_windows_and_table(DEVICE, sizes)


def test_majority_tie_inside_the_event():
    C.case_tie(DEVICE)


def test_label_beyond_its_event_is_refused():
    C.case_bad_label(DEVICE)


def test_spectra_and_scores_per_event():
    C.case_spectra(DEVICE)


def test_spectra_capacity_bounds_every_split():
    from gnn_tracking_amd import _capi

    C.case_capacity(_capi.load())


def test_one_event_is_todays_call():
    C.case_one_event(DEVICE)


def test_performance_details_and_binned_metrics_on_a_collated_batch():
    C.case_scanner(DEVICE)
