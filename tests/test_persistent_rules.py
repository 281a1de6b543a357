"""The host-side rules of the persistent launches (models/engine_config.py): the hand-off error
codes of csrc/kernels/handoff.h as messages, and the co-residency rule the decoder loops and the
graph trainer's BPTT phase share."""
import pytest

from textsummarization_on_flink_amd.models.engine_config import (HANDOFF_CODES, EngineConfig, fits_resident,
                                                                 handoff_error_message)

# (grid, capacity, world, reserve_cus) -> fits
FITS_ROWS = [
    ((256, 256, 1, 0), True),    # grid equal to the capacity, one rank
    ((256, 256, 2, 1), False),   # ... with a CU reserved beside a collective
    ((128, 0, 1, 0), False),     # no device / kernel not admitted
    ((0, 256, 1, 0), False),     # no grid: the shape has no launch
]


def test_handoff_error_message_none_without_error():
    assert handoff_error_message(0) is None


@pytest.mark.parametrize("code, env, field", [(1, "TSAMD_LSTM_PERSISTENT", "persistent_lstm"),
                                              (2, "TSAMD_LSTM_PERSISTENT", "persistent_lstm"),
                                              (3, "TSAMD_DEC_PERSISTENT", "dec_persistent"),
                                              (4, "TSAMD_DEC_BWD_PERSISTENT", "dec_bwd_persistent")])
def test_handoff_error_message_names_switch_and_field(code, env, field):
    msg = handoff_error_message(code)
    assert f"code {code}:" in msg and f"set {env}=0 (EngineConfig.{field})" in msg
    assert HANDOFF_CODES[code][1:] == (env, field) and hasattr(EngineConfig(), field)
    # the switch does switch the field
    assert getattr(EngineConfig.from_env({}), field) and not getattr(EngineConfig.from_env({env: "0"}), field)


def test_handoff_error_message_unknown_code():
    assert handoff_error_message(9)


@pytest.mark.parametrize("args, fits", FITS_ROWS)
def test_fits_resident(args, fits):
    assert fits_resident(*args) is fits


@pytest.mark.parametrize("args", [a for a, _ in FITS_ROWS])
def test_lstm_exclusive_is_not_fits_resident(args):
    """GraphTrainer.__init__ decides lstm_exclusive only with more than one rank and a persistent
    LSTM (a grid); there the earlier expression, grid > capacity - reserve, is ``not fits_resident``."""
    grid, cap, world, reserve = args
    guard = world > 1 and grid > 0
    assert (guard and grid > cap - reserve) == (guard and not fits_resident(grid, cap, world, reserve))
    for g in range(1, 2 * cap + 2, max(1, cap // 8)):  # and for every grid around this capacity
        assert (g > cap - reserve) == (not fits_resident(g, cap, 2, reserve)), (g, cap, reserve)
