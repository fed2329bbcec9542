"""`python train_reader.py --raw-train-data ... --raw-eval-data ... --matched-para-path ...` -- reader training, the
--do_train loop of the reference's qa/train_retrieve_qa.py on one MI355X."""
from proqa_amd.train_reader import main

if __name__ == "__main__":
    main()
