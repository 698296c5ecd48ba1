"""Mirror of the inference-side pieces of ``deephumor.experiments``: the
perplexity metric on the HIP kernels, corpus scoring with per-template encoder caching, and the
text <-> token helpers.  The Trainer / tensorboard harness is out of scope."""
from .metrics import perplexity, sequence_perplexity
from .scoring import CaptionScores, PairScores, explain_captions, score_captions, score_pairs, token_scores
from .occlusion import OcclusionScores, occlusion_maps
from .text_occlusion import TextOcclusionScores, occlusion_to_texts, text_occlusion
from .alternatives import TokenAlternatives, alternatives_to_texts, calibration_table, token_alternatives, topk_accuracy
from .ranking import CaptionRanks, TemplateRanks, rank_captions, rank_templates, template_accuracy
from .inference import attention_to_heatmaps, bad_words_to_ids, beam_logprob_scores, beams_to_texts, group_best, prompts_to_batch, rank_beams, sequence_bias_from_words, text_to_seq, seq_to_text, split_caption

__all__ = ["perplexity", "sequence_perplexity", "score_captions", "text_to_seq", "seq_to_text", "split_caption", "prompts_to_batch",
           "beams_to_texts", "rank_beams", "bad_words_to_ids", "attention_to_heatmaps", "beam_logprob_scores", "group_best",
           "sequence_bias_from_words", "explain_captions", "CaptionScores", "token_scores", "score_pairs", "PairScores",
           "rank_templates", "rank_captions", "template_accuracy", "TemplateRanks", "CaptionRanks",
           "occlusion_maps", "OcclusionScores", "text_occlusion", "TextOcclusionScores", "occlusion_to_texts",
           "token_alternatives", "TokenAlternatives", "alternatives_to_texts", "topk_accuracy", "calibration_table"]
