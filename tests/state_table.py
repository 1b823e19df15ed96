"""What a context holds after a sequence of calls, and which calls it must then accept -- TEST INFRASTRUCTURE shared by
tests/test_state_cpu.py (gaussian_process_amd/csrc/gpmi_state.h against this table, no GPU) and tests/test_state_gpu.py
(the library against it).

The model below is written from the rule as the library documents it, not from the header:

  * at most one fit is resident: a regression factorisation, a binary Laplace fit, a softmax fit or a sparse fit;
    starting any fit replaces whatever was there;
  * another kernel, other lengthscales and another ld_pad drop the fit; a new training set drops the fit and the test set;
  * v (what gpmi_post_chol / gpmi_post_sample need) comes from a regression prediction or a one-pass regression fit, and
    goes with the fit, with a new test set, and when a classifier's prediction reuses its buffer;
  * the posterior-sample factor is kept for the jitter and the v it was made from -- behind L when it rode through the
    augmented factorisation, in a buffer of its own otherwise -- and is never served for another v.

An event that the state does not allow is refused and changes nothing."""

FITS = ("factorize", "fit_predict", "fit_predict_sample", "laplace_fit", "softmax_fit", "sparse_fit")
INVALIDATORS = ("set_kernel", "set_lengthscales", "ld_pad", "set_train")
EVENTS = ("set_train", "set_test", "predict", "laplace_predict", "softmax_predict", "sparse_predict", "post_chol") + FITS + \
    INVALIDATORS[:3]
FIT_OF = {"factorize": "regression", "fit_predict": "regression", "fit_predict_sample": "regression",
          "laplace_fit": "laplace", "softmax_fit": "softmax", "sparse_fit": "sparse"}
# the groups of consumers, and the message of the refusal when the state lacks what the group needs
GROUPS = {"regression": "no factorisation resident", "post": "run gpmi_predict first", "laplace": "no Laplace fit resident",
          "softmax": "no softmax fit resident", "sparse": "no sparse fit resident", "test": "no test set"}
# beside the groups: the posterior-sample factor of the jitter every post_chol here asks for is at hand
POST_KEPT = "post_kept"


class Model:
    def __init__(self):
        self.train = self.test = False
        self.fit = None
        self.v = None             # a serial number per computed v
        self.serial = 0
        self.post_rode = False    # the factor rode through the augmented factorisation that made the current v
        self.post_for = None      # the v the separately kept factor was made from

    def _new_v(self):
        self.serial += 1
        self.v = self.serial

    def _drop_fit(self):
        self.fit = self.v = None
        self.post_rode = False

    def apply(self, ev):
        """-> False when the event is refused"""
        if ev == "set_train":
            self._drop_fit()
            self.train, self.test = True, False
        elif ev in INVALIDATORS:
            self._drop_fit()
        elif ev == "set_test":
            if not self.train:
                return False
            self.test, self.v = True, None
        elif ev in FITS:
            if not self.train or (ev.startswith("fit_predict") and not self.test):
                return False
            self._drop_fit()
            self.fit = FIT_OF[ev]
            if ev.startswith("fit_predict"):
                self._new_v()
                self.post_rode = ev == "fit_predict_sample"
        elif ev == "predict":
            if self.fit != "regression" or not self.test:
                return False
            self._new_v()
            self.post_rode = False
        elif ev in ("laplace_predict", "softmax_predict", "sparse_predict"):
            if self.fit != ev.split("_")[0] or not self.test:
                return False
            if ev != "sparse_predict":
                self.v = None
        elif ev == "post_chol":
            if self.v is None:
                return False
            if not self.post_rode:
                self.post_for = self.v
        else:
            raise ValueError(ev)
        return True

    def accepted(self):
        out = {self.fit} if self.fit else set()
        if self.test:
            out.add("test")
        if self.v is not None:
            out.add("post")
            if self.post_rode or self.post_for == self.v:
                out.add(POST_KEPT)
        return out


def sequences():
    start = ("set_train", "set_test")
    seqs = [start + (a, b) for a in FITS for b in FITS]                          # every ordered pair of fits
    seqs += [start + (a, inv) for a in FITS for inv in INVALIDATORS]             # each fit, then each invalidator
    seqs += [start + (a, "set_test") for a in FITS]                              # a new test set after each fit
    seqs += [("set_train", a, "set_test") for a in FITS]                         # ... and a first one
    # the factor kept for one v is not served for the next
    seqs += [start + ("factorize", "predict", "post_chol", "post_chol", "predict", "post_chol"),
             start + ("fit_predict_sample", "post_chol", "predict", "post_chol", "set_test", "post_chol"),
             start + ("fit_predict", "post_chol", "laplace_fit", "laplace_predict", "factorize", "post_chol", "predict",
                      "post_chol"),
             start + ("factorize", "predict", "post_chol", "softmax_fit", "softmax_predict", "sparse_fit", "sparse_predict")]
    seqs += [("set_test", "factorize", "predict")]                               # nothing without a training set
    return seqs


def expected(seq):
    """-> [accepted set after each event of seq], from a fresh context"""
    m, out = Model(), []
    for ev in seq:
        m.apply(ev)
        out.append(m.accepted())
    return out
