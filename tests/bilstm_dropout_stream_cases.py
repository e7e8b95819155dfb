"""csn_lstm_plan_set_output_dropout in the stream-order tables of tests/stream_order.py (not a test module; it joins the
PLAN_SETTERS table on import, as tests/channel_discovery_stream_cases.py joins the case table).

The setter takes no stream: what it sets swaps the two layout passes of the forward and backward that follow for the masked
instantiations of csrc/lstm_boundary.hip, on the stream of those calls.  BiLSTM sets it on every plan before every forward and
backward (p = 0 on the top layer and outside train() mode), so the module's stream-order test runs those calls with the
setting made between unsynchronised calls; tests/test_gpu_bilstm_dropout.py::test_bilstm_dropout_on_a_side_stream_with_
late_inputs runs the same with p > 0."""
import stream_order as so

so.PLAN_SETTERS.setdefault("csn_lstm_plan_set_output_dropout", ("test_bilstm_module_on_a_side_stream_with_late_inputs",))
