"""`python train_retrieve_qa.py --do_predict ...` -- the reference's qa/train_retrieve_qa.py evaluation command line."""
from proqa_amd.predict_qa import main

if __name__ == "__main__":
    main()
