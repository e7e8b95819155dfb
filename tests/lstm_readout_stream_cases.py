"""csn_lstm_plan_set_readout in the stream-order tables of tests/stream_order.py (not a test module; it joins the
PLAN_SETTERS table on import, as tests/bilstm_dropout_stream_cases.py does), and the case of
tests/test_gpu_lstm_readout.py::test_pooled_calls_on_a_side_stream_with_late_inputs.

The setter takes no stream: what it sets swaps the gather behind the forward's recurrence for the pooling reduction, and on
the backward puts dy_last into the dy_all layout pass (with, for "max", the argmax pre-pass in front of it and a [B, H]
array the plan owns between the two), all on the stream of those calls.  Every module sets it on every plan in front of
every forward and backward ("last" where nothing is pooled), so the BiLSTM stream-order test runs those calls with the
setting made between unsynchronised calls; the case below runs the pooled kernels themselves.

CASE: one state plan of path 0 with lengths (a 0 and a T among them), every input of the forward late behind a Delay and
overwritten behind the call, then the same for the backward's dy_last, dy_all, dh_n and dc_n."""
import stream_order as so

so.PLAN_SETTERS.setdefault("csn_lstm_plan_set_readout", ("test_bilstm_module_on_a_side_stream_with_late_inputs",))

SHAPE = (5, 37, 24, 32, 2)      # B, T, I, H, L
LENGTHS = (37, 0, 1, 36, 20)
MODES = ("mean", "max")
