"""The deterministic word-embedding gradient without a GPU: the additive C ABI (version, chunk, workspace), the
--deterministic flag of the two training commands next to every reference flag, and the keyword of the two modules."""
import inspect

import pytest

from test_train_reader_host import REFERENCE_FLAGS as READER_REFERENCE_FLAGS


@pytest.fixture(scope="module")
def lib():
    from proqa_amd import _lib
    return _lib.load()


def test_abi_version_and_chunk(lib):
    assert lib.proqa_abi_version() == 7
    assert lib.proqa_embed_word_grad_chunk() >= 1


@pytest.mark.parametrize("typed", [0, 1])
@pytest.mark.parametrize("hidden", [128, 768, 1024])
def test_workspace_covers_the_atomic_entry_point_and_grows_with_the_tokens(lib, hidden, typed):
    need = lib.proqa_embed_layernorm_backward_det_workspace_bytes
    existing = (lib.proqa_embed_layernorm_typed_backward_workspace_bytes(hidden) if typed
                else lib.proqa_backward_workspace_bytes(hidden))
    C = lib.proqa_embed_word_grad_chunk()
    sizes = [0, 1, 2, C - 1, C, C + 1, 63, 64, 65, 300, 2047, 2048, 2049, 6580, 40960, 300000, 2 ** 31 - 2]
    values = [need(n, hidden, typed) for n in sorted(set(n for n in sizes if n >= 0))]
    assert values[0] >= existing > 0
    assert all(a <= b for a, b in zip(values, values[1:])) and values[-1] > values[0]
    assert need(6580, hidden, typed) >= existing + 2 * 6580 * 8          # two key buffers of (id, row) at the least
    assert need(6580, hidden, 1) >= need(6580, hidden, 0)


def test_both_parsers_accept_the_flag_and_keep_the_reference_s(lib):
    from proqa_amd import config, train_reader
    parser = config.build_parser()
    flags = {s for a in parser._actions for s in a.option_strings}
    assert {flag for flag, _, _ in config._REFERENCE_FLAGS} <= flags and "--deterministic" in flags
    assert config.get_args([]).deterministic is False
    assert config.get_args(["--deterministic"]).deterministic is True
    assert config.get_args([]).embed_dtype == "auto"
    flags = {s for a in train_reader.build_parser()._actions for s in a.option_strings}
    assert set(READER_REFERENCE_FLAGS) <= flags and {"--index2paraid", "--deterministic"} <= flags
    assert train_reader.get_args([]).deterministic is False
    assert train_reader.get_args(["--deterministic"]).deterministic is True


def test_pretrain_retriever_checks_still_refuse_with_the_flag():
    from proqa_amd import config, pretrain_retriever
    base = ["--train_file", "t.txt", "--predict_file", "d.txt", "--deterministic"]
    assert pretrain_retriever.check_args(config.get_args(base)).deterministic is True
    with pytest.raises(SystemExit):
        pretrain_retriever.check_args(config.get_args(base + ["--local_rank", "0"]))
    with pytest.raises(SystemExit):
        pretrain_retriever.check_args(config.get_args(base + ["--no_cuda"]))


def test_the_modules_and_operators_take_the_keyword_default_off():
    from proqa_amd import trainable
    from proqa_amd.trainable import TrainableRetriever
    from proqa_amd.trainable_reader import TrainableReader
    for fn in (TrainableRetriever.__init__, TrainableReader.__init__, trainable.run_tower, trainable.embed_layernorm_backward,
               trainable.embed_layernorm_typed_backward):
        assert inspect.signature(fn).parameters["deterministic"].default is False, fn
    assert 'getattr(args, "deterministic", False)' in inspect.getsource(TrainableReader.from_args)
