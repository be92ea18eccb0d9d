"""Text <-> token ids for the path's host side (prompt encoding in ``MetaModel.generate``, label building in the dialog
dataset, stop-string matching).  Public surface = what ``MetaModel`` / the dataset / the checkpoint writer call on the
reference's ``accessory.model.tokenizer.Tokenizer``: ``encode(s, bos, eos)``, ``encode_segment``, ``encode_wo_prefix_space``,
``decode``, ``save``, ``n_words``, ``bos_id``, ``eos_id``, ``need_space_before_segment``, ``tokenizer_type``, ``tokenizer``.
Behaviour is pinned by ``tests/golden/meta_tiny.json`` (ids, segment ids, vocabulary facts captured from the reference).

Two vocabularies are supported, each behind a small adapter so that the wrapper itself has no branches:
a SentencePiece ``*.model`` file (Llama) and a HuggingFace tokenizer directory."""
from __future__ import annotations

import os
from pathlib import Path
from typing import List, Optional, Sequence

__all__ = ["Tokenizer", "probe_tokenizer_path_from_pretrained"]


class _SentencePieceVocab:
    kind = "spm"

    def __init__(self, model_file: str):
        from sentencepiece import SentencePieceProcessor
        if not os.path.isfile(model_file):
            raise AssertionError(model_file)
        self.impl = SentencePieceProcessor(model_file=model_file)
        self.bos, self.eos = self.impl.bos_id(), self.impl.eos_id()
        self.size = self.impl.vocab_size()
        assert self.size == self.impl.get_piece_size()

    def ids(self, text: str) -> List[int]:
        return self.impl.encode(text)

    def write(self, directory: str) -> None:
        (Path(directory) / "tokenizer.model").write_bytes(self.impl.serialized_model_proto())

    def pieces(self) -> List[Optional[str]]:
        sp, out = self.impl, []
        for v in range(self.size):
            if sp.is_control(v) or sp.is_unknown(v) or sp.is_unused(v):
                out.append(None)
            elif sp.is_byte(v):
                out.append(_byte_piece(sp.id_to_piece(v)))
            else:
                out.append(sp.id_to_piece(v).replace("\u2581", " "))
        return out


class _HuggingFaceVocab:
    kind = "transformers"

    def __init__(self, directory: str):
        from transformers import AutoTokenizer
        self.impl = AutoTokenizer.from_pretrained(directory, trust_remote_code=True)
        self.eos = self.impl.eos_token_id
        assert self.eos is not None
        self.bos = self.impl.bos_token_id if self.impl.bos_token_id is not None else self.eos
        self.size = len(self.impl)

    def ids(self, text: str) -> List[int]:
        return self.impl.encode(text, truncation=False, add_special_tokens=False)

    def write(self, directory: str) -> None:
        self.impl.save_pretrained(directory)

    def pieces(self) -> List[Optional[str]]:
        special = set(self.impl.all_special_ids)
        toks = self.impl.convert_ids_to_tokens(list(range(self.size)))
        # a byte-level BPE vocabulary spells every byte as one printable character (GPT-2's table: "\u0120" is the space)
        byte_level = any(t is not None and t.startswith("\u0120") for t in toks)
        table = _gpt2_byte_table() if byte_level else None
        out: List[Optional[str]] = []
        for v, t in enumerate(toks):
            if t is None or v in special:
                out.append(None)
            elif byte_level:
                try:
                    out.append(bytes(table[c] for c in t).decode("utf-8"))
                except (KeyError, UnicodeDecodeError):     # an added token, or a piece that ends inside a UTF-8 sequence
                    out.append(None)
            elif len(t) == 6 and t.startswith("<0x") and t.endswith(">"):
                out.append(_byte_piece(t))
            else:
                out.append(t.replace("\u2581", " "))
        return out


def _byte_piece(piece: str) -> Optional[str]:
    """A byte-fallback token ``<0xNN>``: its character when the byte is ASCII, None otherwise (a fragment of a UTF-8 sequence is no
    text on its own)."""
    b = int(piece[3:5], 16)
    return chr(b) if b < 0x80 else None


def _gpt2_byte_table() -> dict:
    """printable character -> byte of byte-level BPE vocabularies (the inverse of GPT-2's bytes_to_unicode)"""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    table, n = {chr(b): b for b in keep}, 0
    for b in range(256):
        if b not in keep:
            table[chr(256 + n)] = b
            n += 1
    return table


def _ends_with(seq: Sequence[int], tail: Sequence[int]) -> bool:
    return len(tail) <= len(seq) and list(seq[len(seq) - len(tail):]) == list(tail)


# single characters that a vocabulary normally keeps as their own token in front of arbitrary text
_SENTINELS = ("@", "\n", "\\", "=", ">", "`")


class Tokenizer:
    def __init__(self, model_path: str):
        self._vocab = _SentencePieceVocab(model_path) if model_path.endswith(".model") else _HuggingFaceVocab(model_path)
        self.tokenizer = self._vocab.impl                 # the wrapped object (the reference exposes it under this name)
        self.tokenizer_type = self._vocab.kind
        self.bos_id: int = self._vocab.bos
        self.eos_id: int = self._vocab.eos
        self.need_space_before_segment = self._segments_need_leading_space()

    # ---- whole strings -------------------------------------------------------------------------------------------
    def encode(self, s: str, bos: bool, eos: bool) -> List[int]:
        assert type(s) is str
        ids = list(self._vocab.ids(s))
        return ([self.bos_id] if bos else []) + ids + ([self.eos_id] if eos else [])

    def decode(self, t: List[int]) -> str:
        return self.tokenizer.decode(t)

    # ---- pieces of a longer string (their ids must equal the ids they get INSIDE that string) -------------------------
    def _segments_need_leading_space(self) -> bool:
        """SentencePiece puts the word-boundary marker on the token AFTER a space, so "my darling" cut out of
        "Hi my darling" encodes identically with or without its own leading space; byte-level BPE vocabularies attach the
        space to the word and need it spelled out.  Probe which kind this is."""
        whole = self._vocab.ids("Hi my darling")
        if _ends_with(whole, self._vocab.ids("my darling")):
            return False
        assert _ends_with(whole, self._vocab.ids(" my darling"))
        return True

    def encode_segment(self, s: str) -> List[int]:
        """ids of a word-initial piece (an answer, a stop string that follows a space)."""
        body = s.lstrip(" ")
        return self.encode(" " + body if self.need_space_before_segment else body, bos=False, eos=False)

    def encode_wo_prefix_space(self, s: str) -> List[int]:
        """ids of a piece that continues a word (no boundary marker on its first token)."""
        if self.need_space_before_segment:
            return self.encode(s, bos=False, eos=False)
        for mark in _SENTINELS:
            head = self._vocab.ids(mark)
            joined = self._vocab.ids(mark + s)
            if list(joined[:len(head)]) == list(head):       # the sentinel survived as its own token(s): drop it
                return list(joined[len(head):])
        raise NotImplementedError(f"All prefixes are merged into {s} during tokenization")

    # ---- bookkeeping ---------------------------------------------------------------------------------------------
    def save(self, save_dir: str) -> None:
        self._vocab.write(save_dir)

    @property
    def n_words(self) -> int:
        return self._vocab.size

    def pieces(self) -> List[Optional[str]]:
        """Per token id the text it contributes to a decoded answer, SentencePiece's word-boundary marker read as a space; ``None``
        for a token that contributes no text (BOS, EOS, pad, unknown, control, a lone byte of a multi-byte character).  The input
        of ``model.constrain.compile_constraint``."""
        return self._vocab.pieces()


def probe_tokenizer_path_from_pretrained(pretrained_path: str) -> Optional[str]:
    """Where a checkpoint directory keeps its vocabulary: ``tokenizer.model`` wins, else an HF pair of json files."""
    root = Path(pretrained_path)
    if (root / "tokenizer.model").is_file():
        return str(root / "tokenizer.model")
    if all((root / name).is_file() for name in ("tokenizer.json", "tokenizer_config.json")):
        return str(pretrained_path)
    return None
