"""train_reader.py without a GPU: the parser, the refusals, the run name, the update schedule with failed retrievals; and
the parser and refusals of train_retrieve_qa.py (predict_qa), which the command's evaluate() was moved out of."""
import pytest

REFERENCE_FLAGS = [
    "--bert_model_name", "--output_dir", "--weight_decay", "--load", "--num_workers", "--train_file", "--predict_file",
    "--init_checkpoint", "--do_lower_case", "--max_seq_length", "--max_query_length", "--do_train", "--do_predict",
    "--train_batch_size", "--predict_batch_size", "--learning_rate", "--adam_epsilon", "--num_train_epochs", "--wait_step",
    "--save_checkpoints_steps", "--iterations_per_loop", "--no_cuda", "--local_rank", "--accumulate_gradients", "--seed",
    "--gradient_accumulation_steps", "--eval_period", "--verbose", "--efficient_eval", "--max_answer_len", "--max_grad_norm",
    "--fp16", "--fp16_opt_level", "--qa-drop", "--rank-drop", "--MI", "--mi-k", "--max-pool", "--eval-workers", "--save-pred",
    "--retriever-path", "--raw-train-data", "--raw-eval-data", "--fix-para-encoder", "--db-path", "--index-path",
    "--matched-para-path", "--use-spanbert", "--spanbert-path", "--eval-k", "--regex", "--separate", "--add-select",
    "--drop-early", "--shared-norm", "--prefix", "--debug", "--use-top-passage", "--topk", "--save-all", "--candidates"]


def _args(*argv):
    from proqa_amd import train_reader
    return train_reader.get_args(list(argv))


def test_the_parser_carries_the_reference_s_flags_and_defaults():
    from proqa_amd import train_reader
    flags = {s for a in train_reader.build_parser()._actions for s in a.option_strings}
    assert set(REFERENCE_FLAGS) <= flags and "--index2paraid" in flags
    a = _args()
    assert (a.train_batch_size, a.learning_rate, a.num_train_epochs, a.eval_period, a.wait_step) == (8, 5e-5, 200, 1000, 100)
    assert (a.max_seq_length, a.max_query_length, a.max_grad_norm, a.seed, a.eval_k, a.qa_drop) == (512, 50, 5.0, 3, 5, 0)
    assert a.index2paraid == "retrieval/index_data/idx_id.json" and a.matched_para_path == "../data/wq_ft_train_matched.txt"
    assert a.do_lower_case is True and a.shared_norm is False and a.drop_early is False and a.fix_para_encoder is False


def test_model_name_is_the_reference_s():
    from proqa_amd import train_reader
    a = _args("--seed", "7", "--train_batch_size", "10", "--prefix", "run", "--learning_rate", "1e-5", "--qa-drop", "0.1",
              "--shared-norm", "--fp16", "--bert_model_name", "bert-base-uncased")
    assert train_reader.model_name(a) == ("dense-seed7-bsz10-fp16True-run-lr1e-05-bert-base-uncased-qdrop0.1-snTrue-sepFalse-"
                                          "asFalse-noearlyFalse")
    assert train_reader.model_name(_args()) == ("dense-seed3-bsz8-fp16False-eval-lr5e-05-bert-base-uncased-qdrop0-snFalse-"
                                                "sepFalse-asFalse-noearlyFalse")


def test_check_args_implies_do_train_and_divides_nothing():
    from proqa_amd import train_reader
    a = train_reader.check_args(_args("--train_batch_size", "10", "--accumulate_gradients", "2"))
    assert a.do_train is True and a.train_batch_size == 10          # the division happens in main, after model_name
    assert train_reader.check_args(_args("--do_train", "--do_predict")).do_train is True


@pytest.mark.parametrize("argv,match", [
    (["--do_predict"], "--do_predict alone"),
    (["--local_rank", "0"], "local_rank"),
    (["--no_cuda"], "no_cuda"),
    (["--use-spanbert"], "use-spanbert"),
    (["--separate"], "separate"),
    (["--add-select"], "add-select"),
])
def test_refusals_are_system_exits(argv, match):
    from proqa_amd import train_reader
    with pytest.raises(SystemExit, match=match):
        train_reader.check_args(_args(*argv))


@pytest.mark.parametrize("argv,match", [
    (["--accumulate_gradients", "0"], "Invalid accumulate_gradients parameter: 0, should be >= 1"),
    (["--train_file", ""], "`train_file` must be specified"),
    (["--predict_file", ""], "`predict_file` must be specified"),
    (["--gradient_accumulation_steps", "0"], "gradient_accumulation_steps"),
    (["--train_batch_size", "2", "--accumulate_gradients", "4"], "passages per question"),
    (["--train_batch_size", "65"], "passages per question"),
    (["--matched-para-path", ""], "matched-para-path"),
])
def test_the_reference_s_value_errors(argv, match):
    from proqa_amd import train_reader
    with pytest.raises(ValueError, match=match):
        train_reader.check_args(_args(*argv))


def test_update_schedule_with_failed_retrievals():
    from proqa_amd.train_reader import update_schedule
    assert update_schedule(6, 2, failed=(1, 4)) == [3, 5]        # the slot of step 1 is used up by the failure
    assert update_schedule(6, 2) == [1, 3, 5]
    assert update_schedule(5, 1, failed=(2,)) == [1, 3, 4, 5]
    assert update_schedule(8, 3, failed=(2, 5)) == [8]           # slots 2, 5, 8
    assert update_schedule(4, 2, failed=(1, 2, 3, 4)) == []
    assert update_schedule(0, 2) == []


def test_train_retrieve_qa_parser_and_refusals_are_unchanged():
    from proqa_amd import predict_qa
    a = predict_qa.build_parser().parse_args(["--do_predict"])
    assert (a.eval_k, a.max_seq_length, a.max_query_length, a.reader_batch, a.search, a.nlist, a.nprobe) == \
        (5, 512, 50, 256, "exact", 100, 20)
    for flag in ("--do_train", "--train_file", "--raw-train-data", "--matched-para-path", "--learning_rate", "--shared-norm",
                 "--fix-para-encoder", "--retriever-path=x"):
        with pytest.raises(SystemExit, match="is not supported: this project runs the reader's evaluation"):
            predict_qa.main([flag])
    with pytest.raises(SystemExit, match="only --do_predict is supported"):
        predict_qa.main([])
    with pytest.raises(SystemExit, match="--search ivf: --eval-k"):
        predict_qa.main(["--do_predict", "--search", "ivf", "--eval-k", "100000"])
    assert callable(predict_qa.evaluate)
