"""The opt-in settings of the generation call, and which of them cannot be combined yet - each stated once.

``OPTIONS`` is the table of the settings that have an environment route (the caller of the unchanged WanVideoGenerator has no
keyword to pass): one row per setting with its keyword (= the pipeline attribute of the same name), its variable and the parser of
the variable's text.  ``from_env`` turns the environment into attribute values (WanVideoPipeline.__init__), ``resolve`` picks keyword
or attribute for one call (WanVideoPipeline.__call__).  What a setting means is its feature module's business: teacache.py,
sliding_window.py, lora.py, v2v.py, attn_window.py, solver.py, guidance.py.

``SCOPE`` is the matrix of combinations that are refused, ``check_scope`` the one place that refuses them.  The pipeline, the engine
(dit.WanDiT) and the generator (inference.WanVideoGenerator) each observe the same conditions in their own terms and name them in
their own words, so the matrix carries no prose: a layer hands ``check_scope`` the strings.

Host logic only; nothing here imports torch.
"""

from __future__ import annotations

from collections import namedtuple

# ---- features, and the conditions that are not features -------------------------------------------------------------------------------
TEACACHE, SLIDING, LORA, V2V, ATTN_WINDOW, SOLVER, CFG_ZERO = "teacache", "sliding_window", "lora", "v2v", "attn_window", "solver", "cfg_zero"
PARALLEL, I2V, FP8_ATTN = "parallel", "i2v", "fp8_attn"      # more than one rank; an image-to-video DiT; e4m3 self-attention

# feature -> the pipeline attribute that holds what the last call did with it (None: the feature was off in that call)
RECORDS = {
    TEACACHE: "tea_cache_record",                 # {"model_id", "thresh", "computed", "distances"}: the skip schedule
    SLIDING: "sliding_window_record",             # [(frame0, frame1), ...]; None also when the clip fitted one window
    LORA: "lora_record",                          # [{path, alpha, matrices, rank}] merged NOW: it outlives a call (pipeline._reconcile_lora)
    V2V: "v2v_record",                            # {"denoising_strength", "sigma_0"}; None: the call started from noise
    ATTN_WINDOW: "attention_window_record",       # {"window", "sink", "key_fraction"}; None also when the window covered the clip
    SOLVER: "solver_record",                      # {"name", "steps", "orders"}; None: Euler steps
    CFG_ZERO: "guidance_record",                  # {"optimized_scale", "zero_init_steps", "scales"}
}


# ---- parsers of a variable's text: parse(variable name, text | None) -> value ---------------------------------------------------------
def integer(what: str, at_least=None, strict: bool = False, default=None):
    """``int()`` of the text.  ``at_least``: a lower bound.  ``strict``: the text must be the number's own decimal spelling (spaces
    around it aside), so '2.5', '+2', '02' and ' ' are refused where plain ``int()`` semantics would take some of them."""
    def parse(name, text):
        if text is None or text == "":
            return default
        try:
            n = int(text)
        except ValueError:
            n = None
        if n is None or (at_least is not None and n < at_least) or (strict and str(n) != text.strip()):
            raise ValueError(f"{name} must be {what}, got {text!r}")
        return n
    return parse


def number(what=None):
    """``float()`` of the text; without ``what`` a bad spelling raises float's own message."""
    def parse(name, text):
        if text is None or text == "":
            return None
        try:
            return float(text)
        except ValueError:
            if what is None:
                raise
            raise ValueError(f"{name} must be {what}, got {text!r}") from None
    return parse


def flag(name, text):
    if text is None or text == "":
        return None
    if text.strip() not in ("0", "1"):
        raise ValueError(f"{name} must be 0 or 1, got {text!r}")
    return text.strip() == "1"


def string(default=None):
    return lambda name, text: text or default


def _loras(name, text):
    from . import lora                  # imports torch: kept out of this module's import
    return [dict(path=p, alpha=a, adapter=None) for p, a in lora.parse_env(text)]


def _given(value) -> bool:
    return value is not None


# ---- the settings -----------------------------------------------------------------------------------------------------------------------
# name: the keyword of WanVideoPipeline.__call__ and the pipeline attribute; env / parse: the variable and its parser; feature + on: the
# feature a value switches on (what the generator asks of a client pipeline); keyword=False: an attribute only
Option = namedtuple("Option", "name env parse feature on keyword", defaults=(None, _given, True))
_frames = integer("an integer number of latent frames")

OPTIONS = (
    Option("tea_cache_l1_thresh", "ICV_TEACACHE_L1_THRESH", number(), TEACACHE),       # step skipping: relative-L1 threshold ...
    Option("tea_cache_model_id", "ICV_TEACACHE_MODEL_ID", string("")),                 # ... and whose polynomial rescales it
    Option("sliding_window_size", "ICV_SLIDING_WINDOW_SIZE", _frames, SLIDING),        # temporal windows, in latent frames ...
    Option("sliding_window_stride", "ICV_SLIDING_WINDOW_STRIDE", _frames, SLIDING),    # ... and their stride
    Option("loras", "ICV_LORA", _loras, LORA, bool, keyword=False),                    # "pathA:0.8,pathB", merged at first use
    Option("input_video", "ICV_INPUT_VIDEO", string(), V2V),                           # video-to-video: a .npy / a directory of images
    Option("denoising_strength", "ICV_DENOISING_STRENGTH", number("a number in (0, 1]"), V2V),
    Option("attention_window_frames", "ICV_ATTN_WINDOW_FRAMES", _frames, ATTN_WINDOW),  # frame-windowed self-attention ...
    Option("attention_sink_frames", "ICV_ATTN_SINK_FRAMES", _frames, ATTN_WINDOW),     # ... plus the clip's first frames
    Option("sample_solver", "ICV_SAMPLE_SOLVER", string(), SOLVER, lambda v: v not in (None, "euler")),
    Option("num_inference_steps", "ICV_SAMPLE_STEPS", integer("an integer >= 1", 1, strict=True, default=50)),   # of ANY solver
    Option("cfg_zero_star", "ICV_CFG_ZERO_STAR", flag, CFG_ZERO, bool),                # CFG-Zero*: the optimised scale ...
    Option("cfg_zero_init_steps", "ICV_CFG_ZERO_INIT_STEPS", integer("an integer >= 0", 0, strict=True), CFG_ZERO, bool),   # ... and zero-init
)

ENV_NAMES = tuple(o.env for o in OPTIONS) + ("ICV_WORLD",)      # everything a test must clear to see the defaults

Call = namedtuple("Call", [o.name for o in OPTIONS if o.keyword])


def from_env(environ) -> dict:
    """{attribute: value} of every option: the variable's parsed text, the option's default where it is unset or empty."""
    return {o.name: o.parse(o.env, environ.get(o.env)) for o in OPTIONS}


def resolve(pipe, keywords) -> Call:
    """The values in effect for one call: the keyword where one is given (not None), else the pipeline's attribute - each setting
    on its own.  ``keywords`` may hold more than the options' names."""
    return Call(*(getattr(pipe, n) if keywords.get(n) is None else keywords[n] for n in Call._fields))


def switched_on(holder) -> set:
    """The features that the attributes of ``holder`` (a pipeline, or a worker pool's client pipeline) switch on."""
    return {o.feature for o in OPTIONS if o.feature is not None and o.on(getattr(holder, o.name, None))}


# ---- what cannot be combined yet -------------------------------------------------------------------------------------------------------
# (feature, condition): the feature that names itself first in the refusal, and what it is refused with.  The relation is symmetric -
# sliding windows exclude the attention window, the multistep solver and CFG-Zero* as much as those exclude sliding windows.  Read by
# rows, in this order; the first pair that holds raises.  Video-to-video never reaches the engine, so only the pipeline and the
# generator observe its row.
SCOPE = (
    (ATTN_WINDOW, SLIDING), (ATTN_WINDOW, FP8_ATTN),
    (SOLVER, SLIDING),
    (CFG_ZERO, SLIDING),
    (SLIDING, PARALLEL), (SLIDING, I2V), (SLIDING, TEACACHE),
    (ATTN_WINDOW, PARALLEL),
    (SOLVER, PARALLEL),
    (CFG_ZERO, PARALLEL),
    (V2V, PARALLEL),
)


def check_scope(active, present) -> None:
    """Refuse the first pair of SCOPE that holds.  ``active``: feature -> how the calling layer names it, for the features that are
    on in this call; ``present``: condition -> how the layer names it, for the conditions that hold - or (feature, condition) -> a
    wording for that one pair.  A false value is the same as a missing key."""
    for feature, condition in SCOPE:
        subject, what = active.get(feature), present.get((feature, condition)) or present.get(condition)
        if subject and what:
            raise ValueError(f"{subject} cannot be combined with {what} yet")
