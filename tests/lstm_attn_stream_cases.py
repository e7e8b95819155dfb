"""csn_lstm_plan_set_attention in the stream-order tables of tests/stream_order.py (not a test module; it joins the
PLAN_SETTERS table on import, as tests/lstm_readout_stream_cases.py does), and the case of
tests/test_gpu_lstm_attn.py::test_attention_calls_on_a_side_stream_with_late_inputs.

The setter takes no stream: what it sets swaps the gather behind the forward's recurrence for the score, row and weighted-sum
kernels, and on the backward puts the score / row pre-passes, the two dq kernels and the attention term of the dy_all layout
pass in front of the recurrence, with [B, T] arrays the plan owns between them -- all on the stream of those calls.  Every
module sets it on every plan in front of every forward and backward (off where no attention is read out), so the BiLSTM
stream-order test runs those calls with the setting made between unsynchronised calls; the case below runs the attention
kernels themselves.

CASE: one state plan of path 0 with lengths (a 0 and a T among them), every input of the forward late behind a Delay and
overwritten behind the call -- the query among them --, then the same for the backward's q, dy_last, dy_all, dh_n and dc_n."""
import stream_order as so

so.PLAN_SETTERS.setdefault("csn_lstm_plan_set_attention", ("test_bilstm_module_on_a_side_stream_with_late_inputs",))

SHAPE = (5, 37, 24, 32, 2)      # B, T, I, H, L
LENGTHS = (37, 0, 1, 36, 20)
